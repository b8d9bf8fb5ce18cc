// shade_class_a.hip — model-class build of the shade kernel: misses (environment emitter), diffuse, dielectric, conductor — with every texture / light / surface-map feature (rough conductor has class g, shade_class_g.hip).
// A scene that needs the full feature set AND has the traversal's key per ray (flattened BVH, dev_scene::flat_leaf_keys) is shaded by one launch per model class present in it
// (kernels.hip launch_shade), each over the slot list k_class_partition made for the class, instead of one kernel over all slots that carries every model and regroups them
// behind workgroup barriers: 256-lane workgroups, full waves of (mostly) one model, no wave that idles at a barrier while the slowest model of the workgroup finishes.
#define CTL_SHADE_NAME class_a
#define CTL_SHADE_FEATURES (0x7F & ~(1 | 2 | 16))
#define CTL_SHADE_KEYS CTL_CLASS_A_KEYS
#define CTL_SHADE_CLASS 0
#ifndef CTL_CLASS_A_BLOCK
#define CTL_CLASS_A_BLOCK 256
#endif
#define CTL_SHADE_BLOCK CTL_CLASS_A_BLOCK
#ifndef CTL_CLASS_A_WAVES
#define CTL_CLASS_A_WAVES 4
#endif
#define CTL_SHADE_WAVES CTL_CLASS_A_WAVES
#include "shade_kernel.inc"
