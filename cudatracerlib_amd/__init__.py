"""cudatracerlib_amd — MI355X-native wavefront path tracer behind the CudaTracerLib tracer-plugin API.

The product is ``libctl_amd.so`` (hand-written HIP for gfx950 + C++ host, C-ABI in ``include/ctl_amd.h``).
This package is a thin ctypes mirror of that C-ABI using the reference's class and method names
(``DynamicScene``, ``Image``, ``WavefrontPathTracer.Resize/InitializeScene/DoPass`` …, Kernel/Tracer.h:67-294).
There is no CPU fallback: without the built extension, importing the API raises.
"""
from .api import (  # noqa: F401
    lib, CtlError, DynamicScene, Scene, Image, Comm, WavefrontPathTracer, PathTracer, PrimTracer, PathTrace_DrawMode, SequenceGenerator,
    ctl_material, ctl_texture, ctl_light, ctl_sensor, ctl_scene_desc, ctl_ray, ctl_hit, ctl_pixel_data,
    ctl_tracer_stats, ctl_traversal_counts, ctl_float4x4,
    diffuse, dielectric, conductor, roughconductor, device_count, intersect, intersect_count, intersect_ex, intersect_pair,
    traversal_stack_histogram, traversal_lds_rows,
    FlatBvh, scene_desc_diff, DIFF_CAMERA, DIFF_MATERIALS, DIFF_LIGHTS, DIFF_TRANSFORMS, DIFF_TOPOLOGY, DIFF_GEOMETRY, skin_mesh_host, shape_sets_host, SKIN_AREA_LIGHTS, mip_pyramid_host, IMAGE_TEXELS_DEVICE,
    DIFF_VOLUMES, ctl_volume, ctl_phase_function, homogeneous_volume, volume_update, volume_eval, volumes_desc,
    VOLUME_HOMOGENEOUS, VOLUME_GRID, ctl_volume_grid, GridVolume, grid_volume, set_desc_volumes,
    phase_isotropic, phase_hg, phase_rayleigh, phase_kajiya_kay,
)
