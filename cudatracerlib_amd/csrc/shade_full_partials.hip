// shade_full_partials.hip — the full-feature shade kernel that computes ray differentials at the first hit and filters image textures there (CTL_TEX_PARTIALS,
// shade_kernel.inc): launched by the WavefrontPathTracer with TextureFiltering = true for the vertices of depth 1, whatever feature set the scene needs (the full
// build is a superset), unclassed like shade_full_media.hip.  PathTrace rules only.
// CTL_PARTIALS_SHADE_BLOCK: 512 lanes = 2 waves per SIMD = 256 VGPRs.  At shade_full.hip's 1024 (128 VGPRs) the partials and mip_eval's call frame push the kernel from
// 89 to 144 spilled registers (1696 B of scratch per lane); at 512 it takes 217 registers and spills none (1360 B of scratch: the BSDF record and the call frames), and
// synthetic-bathroom's depth-1 shade stage is 4 % faster with it (RESULTS.md "First-hit texture filtering in the wavefront").
#define CTL_SHADE_NAME full_partials
#define CTL_SHADE_FEATURES 0x7F
#define CTL_TEX_PARTIALS 1
#ifndef CTL_PARTIALS_SHADE_BLOCK
#define CTL_PARTIALS_SHADE_BLOCK 512
#endif
#define CTL_SHADE_BLOCK CTL_PARTIALS_SHADE_BLOCK
#ifdef CTL_PARTIALS_SHADE_WAVES
#define CTL_SHADE_WAVES CTL_PARTIALS_SHADE_WAVES
#endif
#include "shade_kernel.inc"
