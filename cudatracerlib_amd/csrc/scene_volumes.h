// scene_volumes.h — KernelDynamicScene::m_sVolume of a Scene: the participating media in HBM, a member of the Scene (Scene::volumes_, tracer.h; dev_scene and with it every
// other kernel's arguments stay as they are).  A fixed table of CTL_MAX_VOL_COUNT slots, allocated when the scene is created and written in place by every later
// Scene::snapshot (ctl_scene_update, 0 -> 1 volumes included); its readers, through Scene::volume_table, are the megakernel's MEDIA instantiations (megakernel.hip) and the wavefront's medium path (medium_stage.hip, shade_full_media*.hip).
// Beside it the grid records of the VolumeGrid regions (CTL_MAX_VOL_COUNT slots) and ONE float buffer of their cells, re-uploaded by an update and re-allocated only when it
// grows; the table's g / cells point at them when the scene has a grid region and are null otherwise.
#pragma once
#include "tracer.h"
#include "volume.h"

namespace ctl {

// `host` and `grids` are the host copies the snapshot's `volumes` / `volume_grids` point at, the data pointers of `grids` into `pack.cells` (the floats as the device holds them)
struct scene_volumes {
    dbuf<ctl_volume> dev; std::vector<ctl_volume> host; vol::table T{};
    dbuf<vol::grid_rec> dev_grids; dbuf<float> dev_cells; vol::grid_pack pack; std::vector<ctl_volume_grid> grids;
    scene_volumes();   // both tables allocated and zeroed: no media
    // the description's media into the tables, synchronously, where they differ from what is held; returns `host` (null without media) and, in `grids_out`, `grids`
    const ctl_volume* store(const ctl_scene_desc& d, const ctl_volume_grid** grids_out);
};

}  // namespace ctl
