// shade_full_media_grid.hip — shade_full_media.hip for a volume table that holds a VolumeGrid region (CTL_SHADE_MEDIA 2): the transmittance of the surface NEE
// dispatches on the region type and marches the density grids (volume_grid.h).  Launched only for such a table, so that the homogeneous build carries no march.
#define CTL_SHADE_NAME full_media_grid
#define CTL_SHADE_FEATURES 0x7F
#define CTL_SHADE_MEDIA 2
#define CTL_SHADE_BLOCK 1024
#include "shade_kernel.inc"
