// scene_volumes.h — KernelDynamicScene::m_sVolume of a Scene: the participating media in HBM, kept BESIDE the Scene object (scene_update.hip) so that dev_scene, the
// Scene class and with them every other kernel's arguments stay as they are.  A fixed table of CTL_MAX_VOL_COUNT slots per scene, allocated when the scene is created and
// written in place by ctl_scene_update (0 -> 1 volumes included); its only readers are the megakernel's MEDIA instantiations (megakernel.hip).  Beside it, per scene, the grid
// records of the VolumeGrid regions (CTL_MAX_VOL_COUNT slots) and ONE float buffer of their cells, re-uploaded by an update and re-allocated only when it grows; the table's
// g / cells point at them when the scene has a grid region and are null otherwise.
#pragma once
#include "volume.h"

namespace ctl {

class Scene;
vol::table scene_volume_table(const Scene* s);   // n == 0: no media (also for a scene the registry does not know)
// a number that names the scene for as long as it lives (0: unknown to the registry): a holder of a Scene* that may outlive the scene tells a new scene at the same
// address from the one it was given
uint64_t scene_volumes_id(const Scene* s);
// the plugins without medium code refuse a scene that has media instead of rendering it without them: unsupported_error naming `who` and the PathTracer plugin
void refuse_volumes(const Scene* s, const char* who);

}  // namespace ctl
