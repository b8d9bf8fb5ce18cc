// shade_full_media.hip — the full-feature shade kernel for a scene with homogeneous participating media (CTL_SHADE_MEDIA 1, shade_kernel.inc): launched by the
// WavefrontPathTracer with ParticipatingMedia = true behind k_medium_stage, whatever feature set the scene needs (the full build is a superset).  PathTrace rules only.
// Workgroup size as shade_full.hip.
#define CTL_SHADE_NAME full_media
#define CTL_SHADE_FEATURES 0x7F
#define CTL_SHADE_MEDIA 1
#define CTL_SHADE_BLOCK 1024
#include "shade_kernel.inc"
