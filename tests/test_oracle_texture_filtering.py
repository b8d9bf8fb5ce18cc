"""The yardstick of tests/test_gpu_texture_filtering.py is the oracle's render(..., partials=True).  Those tests hold a frame rendered with TextureFiltering = true to it;
they would pass vacuously on a scene whose frame the partials do not change.  Here, without a GPU: on each of their scenes the oracle's frames with and without
partials differ in at least 10 % of the pixels (at the per-pixel bar the GPU tests use, 2e-3 (1 + ref))."""
import numpy as np
import pytest
import filtering_scenes as F


def _differ(a, b):
    return 1.0 - (np.abs(a[..., :3] - b[..., :3]) <= 2e-3 * (1 + np.abs(b[..., :3]))).all(axis=2).mean()


# (spherical, anisotropic) is the one pair left out of the 10 % bar: SphericalSensor::sampleRayDifferential sets the ray only, so the differential rays ARE the ray,
# computePartials returns zero derivatives and KernelMIPMap::eval's EWA branch, handed a zero-width footprint, returns the bilinear level-0 lookup — the frame of the
# plain lookup, asserted below.  The trilinear filter under the same sensor does differ (it goes through its own level selection), and that pair is in the GPU tests.
CASES = [(s, f) for s in F.SENSORS for f in ("anisotropic", "trilinear") if (s == "perspective" or f == "anisotropic" or s == "spherical")]


@pytest.mark.parametrize("sensor,filter_mode", CASES)
def test_partials_change_the_ground_frames(orc, sensor, filter_mode):
    """the scenes of the grazing-ground, plugin-agreement, batch / shard (perspective, both filters) and every-sensor tests: 96 x 64, 2 passes, depth 3"""
    sc = F.ground_scene(filter_mode, sensor)
    tables = orc.sequence_tables(2)
    plain, _ = orc.render(sc.desc, F.W, F.H, n_passes=2, tables=tables, max_path_length=3)
    filtered, _ = orc.render(sc.desc, F.W, F.H, n_passes=2, tables=tables, max_path_length=3, partials=True)
    assert np.array_equal(plain[..., 6], filtered[..., 6])
    if (sensor, filter_mode) == ("spherical", "anisotropic"):
        assert np.array_equal(plain, filtered)
        return
    assert _differ(filtered, plain) >= 0.10, _differ(filtered, plain)


def test_partials_change_the_block_sampler_frame(orc):
    """the scene of the second-sample test: thin lens, 128 x 128 (2 x 2 blocks), one pass with 0 / 1 / 2 samples per block — the ground fills the lower two blocks"""
    sc = F.ground_scene("anisotropic", "thinlens", F.BW, F.BH)
    tables = orc.sequence_tables(1)
    counts = np.array([[1, 0], [2, 1]], np.uint8)
    plain, _ = orc.render(sc.desc, F.BW, F.BH, n_passes=1, tables=tables, max_path_length=3, block_counts=counts)
    filtered, _ = orc.render(sc.desc, F.BW, F.BH, n_passes=1, tables=tables, max_path_length=3, block_counts=counts, partials=True)
    assert np.array_equal(plain[..., 6], filtered[..., 6]) and plain[64:, :64, 6].mean() > 1.9 and plain[:64, 64:, 6].sum() < 0.02 * 64 * 64
    assert _differ(filtered, plain) >= 0.10, _differ(filtered, plain)
    assert _differ(filtered[64:, :64], plain[64:, :64]) >= 0.10      # the block whose pixels draw a second sample
