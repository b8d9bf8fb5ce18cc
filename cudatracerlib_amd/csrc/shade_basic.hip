// shade_basic.hip — shade kernel for scenes that only use the BSDFs, textures and emitters of the basic feature set (shading.h).
// CTL_BASIC_SHADE_BLOCK / CTL_BASIC_SHADE_WAVES: workgroup size and waves per SIMD the register allocation is held to (measured choices, EXPERIMENTS.md):
// 256-lane workgroups — the three barriers of block_append3 then stall one workgroup of a CU's four or five, not half of the CU
// (round 5, with the LDS tables, shade ms per pass on synthetic-SM, workgroup / regroup window: 512 / 128 1.359, 256 / 128 1.363, 256 / 256 1.326 (and the traversal of the
// next bounce 4.92 against 4.97: its queue order), 512 / 256 1.38, 512 / 512 1.40; profiles/r05t_shade_block_window.jsonl).
// Five waves per SIMD = 96 VGPRs, five workgroups per CU.  The kernel is latency-bound, so a fifth wave pays — as long as it costs no spills: round 5's "5 waves per SIMD: 1.70 ms"
// (against 1.33 at four) was a build with 47 spill stores and 65 reloads in 116 B of scratch, and a reload goes through the vector-memory counter in front of which every
// queued load waits.  Without the SLP vectoriser (build.py) and with the long-lived words parked in LDS (CTL_SHADE_PARK, shade_kernel.inc: 12 KB per workgroup) the kernel has
// 96 VGPRs and no scratch: 1.243 ms against 1.275 at four waves without parking and 1.351 before (one box, profiles/r17a_ab.txt; tests/test_kernel_resources.py holds the
// allocation).  Six waves do not fit: five workgroups of 29 644 B fill the CU's 160 KB of LDS, and with fewer words parked the 80-VGPR build spills (96 B of scratch).
#define CTL_SHADE_NAME basic
#define CTL_SHADE_FEATURES 0
#ifndef CTL_BASIC_SHADE_BLOCK
#define CTL_BASIC_SHADE_BLOCK 256
#endif
#define CTL_SHADE_BLOCK CTL_BASIC_SHADE_BLOCK
#ifndef CTL_BASIC_SHADE_WAVES
#define CTL_BASIC_SHADE_WAVES 5
#endif
#define CTL_SHADE_WAVES CTL_BASIC_SHADE_WAVES
#ifndef CTL_BASIC_SORT_WINDOW
#define CTL_BASIC_SORT_WINDOW 256   // round 4: lanes regroup by BSDF model inside windows of 128 slots (round 5: 256, with 256-lane workgroups), keyed by the byte the closest-hit traversal leaves per ray (dev_scene::hit_key_out): shade 1.52 -> 1.47 ms per
                                   // pass on synthetic-SM (256: 1.48; 512: 1.52 — a wider window packs the rough-conductor lanes better and scatters the path-state reads more; 0 = off: 1.52).  With the key
                                   // derived in the kernel (hit -> node -> triangle -> material: four dependent loads) the regrouping LOST 11 % in round 2.  The model-ordered slot lists of
                                   // the class builds (k_class_partition, 16384-slot windows, 256-lane workgroups) lose here: 2.21 ms — this kernel is bound by its path-state streams, and a list
                                   // turns them into gathers (profiles/r04_shade_experiments.log)
#endif
#define CTL_SHADE_SORT_WINDOW CTL_BASIC_SORT_WINDOW
#ifndef CTL_BASIC_SHADE_PARK
#define CTL_BASIC_SHADE_PARK 1
#endif
#define CTL_SHADE_PARK CTL_BASIC_SHADE_PARK
#define CTL_SHADE_GRID_WAVES CTL_BASIC_SHADE_WAVES
#include "shade_kernel.inc"
