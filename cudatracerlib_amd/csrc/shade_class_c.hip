// shade_class_c.hip — model-class build of the shade kernel: the nesting models — coating, rough coating, blend — whose inner model can be any other (all models compiled in, the inner calls out of line).
// A scene that needs the full feature set AND has the traversal's key per ray (flattened BVH, dev_scene::flat_leaf_keys) is shaded by one launch per model class present in it
// (kernels.hip launch_shade), each over the slot list k_class_partition made for the class, instead of one kernel over all slots that carries every model and regroups them
// behind workgroup barriers: 256-lane workgroups, full waves of (mostly) one model, no wave that idles at a barrier while the slowest model of the workgroup finishes.
#define CTL_SHADE_NAME class_c
#define CTL_SHADE_FEATURES 0x7F
#define CTL_SHADE_KEYS CTL_CLASS_C_KEYS
#define CTL_SHADE_CLASS 2
#define CTL_SHADE_MODELS 0xFFFFu   // every model: a coating's or a blend's inner model can be any
#ifndef CTL_CLASS_C_BLOCK
#define CTL_CLASS_C_BLOCK 256
#endif
#define CTL_SHADE_BLOCK CTL_CLASS_C_BLOCK
#ifndef CTL_CLASS_C_WAVES
#define CTL_CLASS_C_WAVES 4
#endif
#define CTL_SHADE_WAVES CTL_CLASS_C_WAVES
#include "shade_kernel.inc"
