// volume_eval.h — the C++ halves of ctl_volume_update and ctl_volume_eval (volume_eval.hip); both throw std::runtime_error
#pragma once
#include "../../include/ctl_amd.h"
#include "volume.h"

namespace ctl {

void volume_update(ctl_volume& v);   // the derived fields: world_to_volume, the Kajiya-Kay normalisation
void volume_eval(const ctl_scene_desc& d, int what, const float* queries, uint32_t n, float* out, bool on_device);

}  // namespace ctl
