// shading_eval_partials.hip — ctl_shading_eval, build 2: the full feature set with first-hit uv partials and filtered texture lookups, tables in global memory:
// the configuration of megakernel.hip / prim_tracer.hip.
#define CTL_EVAL_NAME partials
#define CTL_SHADE_FEATURES 0x7F
#define CTL_SHADE_MODELS 0xFFFFu
#define CTL_TEX_PARTIALS 1
#include "shading_eval.inc"
