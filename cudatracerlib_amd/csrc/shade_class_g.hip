// shade_class_g.hip — model-class build of the shade kernel: rough conductor alone (kernels.h CTL_CLASS_G_KEYS), with every texture / light / surface-map feature.
// A scene that needs the full feature set AND has the traversal's key per ray (flattened BVH, dev_scene::flat_leaf_keys) is shaded by one launch per model class present in it
// (kernels.hip launch_shade), each over the slot list k_class_partition made for the class, instead of one kernel over all slots that carries every model and regroups them
// behind workgroup barriers: 256-lane workgroups, full waves of (mostly) one model, no wave that idles at a barrier while the slowest model of the workgroup finishes.
#define CTL_SHADE_NAME class_g
#define CTL_SHADE_FEATURES (0x7F & ~(1 | 2 | 16))
#define CTL_SHADE_KEYS CTL_CLASS_G_KEYS
#define CTL_SHADE_CLASS 4
#ifndef CTL_CLASS_G_BLOCK
#define CTL_CLASS_G_BLOCK 256
#endif
#define CTL_SHADE_BLOCK CTL_CLASS_G_BLOCK
#ifndef CTL_CLASS_G_WAVES
#define CTL_CLASS_G_WAVES 4
#endif
#define CTL_SHADE_WAVES CTL_CLASS_G_WAVES
#include "shade_kernel.inc"
