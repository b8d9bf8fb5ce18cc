// scene_checks.h — what makes a ctl_scene_desc one the device code can take: every refusal that needs nothing but the description.  ctl_scene_create, ctl_scene_update
// and ctl_scene_desc_check all call this, before anything is written; which BSDF models and shade features exist is device_scene.h's knowledge.
#pragma once
#include "../../include/ctl_amd.h"

namespace ctl {

constexpr uint32_t kCheckAllParts = CTL_DIFF_CAMERA | CTL_DIFF_MATERIALS | CTL_DIFF_LIGHTS | CTL_DIFF_TRANSFORMS | CTL_DIFF_TOPOLOGY | CTL_DIFF_VOLUMES;   // what creation checks

// Throws std::runtime_error(who + ": " + what) for the first rule that `d` breaks among the rules of `parts` (CTL_DIFF_* bits: an update passes the mask it found,
// whose other parts are those of a description that was checked already):
//   CTL_DIFF_TOPOLOGY    a scene has nodes, a node names a mesh — only creation can meet these, and CTL_DIFF_TOPOLOGY in `parts` says that creation is asking
//   CTL_DIFF_TRANSFORMS  affine node transforms; the scene BVH fits the traversal stack next to the deepest mesh BVH (check_traversal_stack)
//   CTL_DIFF_GEOMETRY    the mesh BVHs next to the scene BVH on the traversal stack (check_traversal_stack): what creation checks of the arrays a geometry update brings
//   CTL_DIFF_LIGHTS      env_map_index, light types, the lights' image indices
//   CTL_DIFF_MATERIALS   texture types and image indices, map kind, alpha state, BSDF type, nested BSDFs, distributions and their transmittance tables
//   CTL_DIFF_CAMERA      the sensor type
//   CTL_DIFF_VOLUMES     at most CTL_MAX_VOL_COUNT volumes; finite, non-negative coefficients; a finite matrix with a finite inverse; a known phase function, |g| < 1,
//                        finite Kajiya-Kay terms (creation checks these too)
// What needs the flattened tree (a leaf's material index, the flattened depth, the node format) is checked where the tree is made (tracer.hip).
void check_scene_desc(const ctl_scene_desc& d, uint32_t parts, const char* who);

// The two-level traversal keeps (scene-BVH depth + exit marker + mesh-BVH depth) entries on its per-lane stack of kStackSize: child links that form no cycle and a
// depth that fits.  strict_top_level: a scene-BVH link or start node outside the array, or a leaf that names a missing node, is refused — an update does; creation
// walks past such links as it always did (they are never followed on the host, and tightening creation would refuse descriptions it takes today).
void check_traversal_stack(const ctl_scene_desc& d, bool strict_top_level, const char* who);

}  // namespace ctl
