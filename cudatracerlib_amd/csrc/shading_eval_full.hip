// shading_eval_full.hip — ctl_shading_eval, build 1: every BSDF, texture and emitter type, the transcendental functions out of line, the scene's small tables in
// LDS.  The feature set and the tables are shade_full's; the out-of-line math (CTL_FMATH_OUTLINE) is what shade_kernel.inc adds for the model-class builds (shade_class_c).
#define CTL_EVAL_NAME full
#define CTL_SHADE_FEATURES 0x7F
#define CTL_SHADE_MODELS 0xFFFFu
#define CTL_FMATH_OUTLINE
#define CTL_SHADE_LDS_TABLES 12
#include "shading_eval.inc"
