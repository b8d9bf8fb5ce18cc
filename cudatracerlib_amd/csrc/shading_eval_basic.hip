// shading_eval_basic.hip — ctl_shading_eval, build 0: the shading functions as shade_basic.hip compiles them (the default workload's shade kernel): the basic feature
// set with shade_kernel.inc's LDS tables.
#define CTL_EVAL_NAME basic
#define CTL_SHADE_FEATURES 0
#define CTL_SHADE_LDS_TABLES 12
#include "shading_eval.inc"
