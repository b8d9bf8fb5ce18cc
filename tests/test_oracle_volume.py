"""Participating media against the reference's OWN code (no GPU): SceneTypes/Volumes.cu and SceneTypes/PhaseFunction.cu built whole from the reference's sources, and
PathTrace<DIRECT> with a bound volume aggregate (oracle/Makefile, oracle/ref_volume_driver.cpp, oracle/ref_pathtrace_driver.cpp), recorded in
tests/golden/volumes.npz and tests/golden/pathtrace_media.npz by tests/golden/generate.py (sections `volumes` and `pathtrace_media`).

Two things are held to the fixtures:
  * the numpy restatement tests/volume_ref.py — the yardstick of tests/test_volume_host.py and tests/test_gpu_volume.py — run with glibc's transcendental functions
    (oracle.Oracle(), as the reference compiled for the host runs them): every sent row of every function BIT FOR BIT, NaN for NaN, and every frame bit for bit;
  * the host yardstick ctl_volume_eval(on_device = 0) (csrc/volume.h with csrc/ctl_fmath.h) directly: discrete outputs equal, float outputs within a per-function
    ulp bound that is twice the measured distance of the glibc and the shared-math restatement over the same rows (neither is code under test).

Where the reference's behaviour is undefined it was never run, and the fixture says where (media section):
  1. sampleVolume with several regions indexes m_pVolumes with ffsn's bit MASK; a row in which that index lies past the table is not sent (`*_sent`, at most 25 % of a
     function's rows on a set; none on the set `four`), and `sixteen` is recorded only for the functions that do not go through sampleVolume;
  2. PathTrace's MediumSamplingRecord is an uninitialised local: the per-function driver zero-fills it, and the frames are cases in which no pixel reads it unwritten;
  3. PathTrace's last_nor is an uninitialised local too (Integrators/PathTracer.cu:21), read by the emission MIS weight (:71) when a path reaches an emitter with Direct
     on after medium vertices only: the frames are rendered with a window of the sampler's table sequence in which no pixel does that (generate.pathtrace_media_cases).
One more place changes no radiance but the number of rays: once a path's throughput is exactly zero the reference walks on (the product ends it) along a direction
nothing has set — pRec.wo after KernelAggregateVolume::Sample found no region (Volumes.cu:297-305; PathTracer.cu:50-53), or the BSDF record's previous wo after a failed
sample (PathTracer.cu:79-85).  Every frame is compared in EVERY pixel (rgb sums and weightSum); ray counts are compared bit for bit in the pixels whose samples never
reached a zero throughput, and in the others the reference must have traced at least the rays up to that point.
Reads only the fixtures and the product's host code."""
import os
import sys

import numpy as np
import pytest

import volume_cases as K
import volume_ref
from cudatracerlib_amd import api

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REGEN_ROWS = "the volume sets changed: regenerate tests/golden/volumes.npz (python tests/golden/generate.py volumes)"
REGEN_FRAMES = "the compiled scene, its volumes or the sampler tables changed: regenerate tests/golden/pathtrace_media.npz (python tests/golden/generate.py pathtrace_media)"

# Discrete outputs (column 0 of the result row): hit, success, region index
DISCRETE = (api.VEVAL_REGION_INTERSECT, api.VEVAL_INTERSECT, api.VEVAL_REGION_SAMPLE_DISTANCE, api.VEVAL_SAMPLE_DISTANCE, api.VEVAL_SAMPLE_VOLUME)
# MEASURED[what]: the largest distance in ulp between the glibc and the shared-math restatement (volume_ref with oracle.Oracle() / Oracle(shared_math=True)) over all
# sent rows and all sets of the fixture (RESULTS.md, media); the bound on the host and the device yardstick against the fixture is twice that.  The functions without a
# transcendental call (IntersectP, tau, sampleVolume, Evaluate of HG / isotropic / Rayleigh, p) measure 0: there the yardstick must equal the reference bit for bit.
# The large figures of the two Sample functions are components of wo close to zero (sinTheta * cosPhi under cancellation), not large errors.
MEASURED = {api.VEVAL_REGION_INTERSECT: 0, api.VEVAL_INTERSECT: 0, api.VEVAL_REGION_TAU: 0, api.VEVAL_TAU: 0, api.VEVAL_REGION_SAMPLE_DISTANCE: 3, api.VEVAL_SAMPLE_DISTANCE: 1,
            api.VEVAL_SAMPLE_VOLUME: 0, api.VEVAL_PHASE_EVAL: 0, api.VEVAL_PHASE_SAMPLE: 32, api.VEVAL_P: 0, api.VEVAL_SAMPLE: 8, api.VEVAL_TRANSMITTANCE: 1,
            api.VEVAL_EVAL_TRANSMITTANCE: 0}
ULP_BOUND = {what: 2 * m for what, m in MEASURED.items()}
DISCRETE_SHARE_CAP = 0.005   # rows in which the two restatements themselves disagree on a discrete output
KK_MEASURED = 0              # glibc against shared-math restatement of KajiyaKayPhaseFunction::Update's 999-term sum, in ulp, over the exponents of the sets
KK_BOUND = 2 * KK_MEASURED

_memo = {}


def _generate():
    sys.path.insert(0, G)
    import generate
    return generate


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(G, "volumes.npz"))


@pytest.fixture(scope="module")
def frames():
    return np.load(os.path.join(G, "pathtrace_media.npz"))


def ulps(a, b):
    """distance in units in the last place, element by element; NaN against NaN is 0, NaN against a number is huge"""
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    ia = a.view(np.int32).astype(np.int64); ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia); ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.where(np.isnan(a) & np.isnan(b), 0, np.where(np.isnan(a) | np.isnan(b), 1 << 40, np.abs(ia - ib)))


def case_rows(golden, orc_libm, orc_sm, what, name):
    """the fixture's rows of one (function, set), with the two restatements' rows over the same queries; computed once per module"""
    k = (what, name)
    if k not in _memo:
        vols = K.make_set(name)
        assert K.table_digest(vols) == str(golden[name + "_digest"]), REGEN_ROWS
        key = "%d_%s" % (what, name)
        q, want, sent = golden[key + "_q"], golden[key + "_out"], golden[key + "_sent"].astype(bool)
        assert np.array_equal(q, K.queries(name, vols, what, K.GOLDEN_ROWS)), REGEN_ROWS
        V = volume_ref.Volumes(orc_libm, K.with_normalization(vols, golden[name + "_kk_normalization"]))   # the reference's own normalisation, as its constructor made it
        _memo[k] = dict(vols=vols, q=q, want=want, sent=sent, V=V, glibc=volume_ref.eval_rows(V, what, q), sm=volume_ref.eval_rows(volume_ref.Volumes(orc_sm, vols), what, q))
    return _memo[k]


def sets_of(what):
    return [name for w, name in K.golden_pairs() if w == what]


@pytest.mark.parametrize("what", sorted(K.FUNCTIONS))
def test_restatement_with_glibc_equals_the_references_own_volumes(golden, _orc_libm, orc_sm, what):
    """volume_ref.Volumes(oracle.Oracle(), ...) against the reference's own functions: every sent row bit for bit, NaN for NaN; and the sent-mask is the one the
    restatement's sampleVolume dictates (an index past the table), recomputed here"""
    for name in sets_of(what):
        c = case_rows(golden, _orc_libm, orc_sm, what, name)
        sent, masks = K.sent_mask(c["V"], what, c["q"])
        assert np.array_equal(sent.astype(bool), c["sent"]), (K.FUNCTIONS[what], name)
        bad = [i for i in K.same_rows(c["glibc"], c["want"]) if c["sent"][i]]
        assert not bad, "%s on set %s: %d of %d sent rows differ from the reference, first %s\n  got %s\n want %s\nquery %s" % (
            K.FUNCTIONS[what], name, len(bad), int(c["sent"].sum()), bad[0], c["glibc"][bad[0]], c["want"][bad[0]], c["q"][bad[0]])
        assert not c["want"][~c["sent"]].any()


def against_fixture(c, what, name, got, who):
    """discrete outputs equal and float outputs within ULP_BOUND[what] of the fixture, over the sent rows in which the two restatements agree on the discrete output;
    returns (rows compared, rows set aside, largest distance seen)"""
    rows = c["sent"].copy(); aside = 0
    if what in DISCRETE:
        differ = c["sent"] & (c["glibc"][:, 0] != c["sm"][:, 0])
        aside = int(differ.sum()); rows &= ~differ
        bad = np.nonzero(rows & (got[:, 0] != c["want"][:, 0]))[0]
        assert not len(bad), "%s %s on set %s: discrete output differs in row %d: %s against %s" % (who, K.FUNCTIONS[what], name, bad[0], got[bad[0]], c["want"][bad[0]])
    d = ulps(got[rows], c["want"][rows])
    worst = int(d.max()) if d.size else 0
    assert worst <= ULP_BOUND[what], "%s %s on set %s: %d ulp from the reference, bound %d; row %d" % (who, K.FUNCTIONS[what], name, worst, ULP_BOUND[what], int(np.nonzero(rows)[0][np.argmax(d.max(axis=1))]))
    return int(rows.sum()), aside, worst


@pytest.mark.parametrize("what", sorted(K.FUNCTIONS))
def test_host_yardstick_against_the_references_own_volumes(golden, _orc_libm, orc_sm, what):
    """ctl_volume_eval(on_device = 0) against the fixture directly.  The distance of the two restatements is measured again here and must not exceed the figure the bound
    was derived from (MEASURED); the share of rows in which they disagree on a discrete output stays under 0.5 %."""
    n = aside = 0; measured = 0
    for name in sets_of(what):
        c = case_rows(golden, _orc_libm, orc_sm, what, name)
        agree = c["sent"] & ((c["glibc"][:, 0] == c["sm"][:, 0]) if what in DISCRETE else True)
        measured = max(measured, int(ulps(c["sm"][agree], c["glibc"][agree]).max()))
        host = api.volume_eval(api.volumes_desc(c["vols"]), what, c["q"], on_device=False)
        a, b, worst = against_fixture(c, what, name, host, "host")
        n += a; aside += b
        print("%s on %s: %d rows, %d set aside, host %d ulp from the reference (bound %d)" % (K.FUNCTIONS[what], name, a, b, worst, ULP_BOUND[what]))
    print("%s: glibc against shared-math restatement %d ulp (recorded %d)" % (K.FUNCTIONS[what], measured, MEASURED[what]))
    assert measured <= MEASURED[what], "the measured distance grew: %d ulp, the bound was derived from %d" % (measured, MEASURED[what])
    assert aside <= DISCRETE_SHARE_CAP * (n + aside), (aside, n)


def test_kajiya_kay_normalization_against_the_references_own(golden, _orc_libm, orc_sm):
    """ctl_volume_update's normalisation against KajiyaKayPhaseFunction's own m_normalization (its constructor's Update(), PhaseFunction.cu:78-93); the glibc restatement
    of the sum equals it bit for bit"""
    n = 0
    for name in K.GOLDEN_SETS:
        for v, want in zip(K.make_set(name), golden[name + "_kk_normalization"]):
            if v.phase.type != api.PHASE_KAJIYA_KAY:
                assert want == 0
                continue
            e = np.float32(v.phase.exponent)
            glibc = volume_ref.kajiya_kay_normalization(volume_ref.Math(_orc_libm), e); sm = volume_ref.kajiya_kay_normalization(volume_ref.Math(orc_sm), e)
            assert glibc.view(np.uint32) == np.float32(want).view(np.uint32), (name, glibc, want)
            measured = int(ulps([sm], [glibc])[0]); got = int(ulps([np.float32(v.phase.normalization)], [want])[0])
            print("Kajiya-Kay exponent %g: glibc against shared-math restatement %d ulp, ctl_volume_update %d ulp from the reference" % (e, measured, got))
            assert measured <= KK_MEASURED and got <= KK_BOUND, (name, measured, got)
            n += 1
    assert n >= 3


@pytest.mark.parametrize("key", [c[0] for c in _generate().pathtrace_media_cases() if not c[0].startswith("clear")])
def test_restatement_path_trace_equals_the_references_own_path_trace(frames, _orc_libm, key):
    """volume_ref.path_trace(oracle.Oracle(), ..., reference_rules=True) against the reference's PathTrace with media: rgb sums and weightSum bit for bit in every pixel;
    rays as the module's docstring says; and the restatement counts no read of unwritten memory in any pixel (the condition under which the case was recorded)"""
    generate = _generate()
    _, make, w, h, direct, first = next(c for c in generate.pathtrace_media_cases() if c[0] == key)
    sc = make(); d = sc.desc
    tables = generate.pathtrace_media_tables(first)
    assert generate.pathtrace_media_digest(d, tables) == str(frames[key + "_digest"]), REGEN_FRAMES
    rays = np.zeros((h, w), np.uint32); undefined = np.zeros((h, w, 6), np.int32)
    img = volume_ref.path_trace(_orc_libm, d, generate.media_volumes(d), w, h, tables, direct=direct, max_path_length=generate.MEDIA_MAX_PATH_LENGTH, rr_start=generate.MEDIA_RR_START,
                                reference_rules=True, pixel_rays=rays, undefined=undefined)
    assert not undefined[..., :3].any(), "the case reaches undefined behaviour of the reference: %s" % undefined.reshape(-1, 6).sum(axis=0)[:3]
    rgb, weight, want_rays = frames[key + "_rgb"], frames[key + "_weight"], frames[key + "_rays"].astype(np.uint32)
    same = np.all(img[..., :3].view(np.uint32) == rgb.view(np.uint32), axis=2) & (img[..., 6].view(np.uint32) == weight.view(np.uint32))
    assert same.all(), "%s: %d pixels differ from the reference's PathTrace, first %s" % (key, (~same).sum(), np.argwhere(~same)[:5].tolist())
    assert (img[..., 3:6] == 0).all()
    walked = undefined[..., 4] > 0   # some sample of the pixel reached a zero throughput: the reference walks on along a direction nothing has set
    bad = (rays != want_rays) & ~walked
    print("%s: rays compared exactly in %d of %d pixels" % (key, (~walked).sum(), w * h))
    assert not bad.any(), "%s: ray counts differ in %d pixels, first %s" % (key, bad.sum(), np.argwhere(bad)[:5].tolist())
    assert (want_rays >= rays - undefined[..., 5].astype(np.uint32)).all()
    assert (~walked).sum() >= 32, "too few pixels to hold the ray counts to"


def test_media_fixture_covers_the_rule_sets(golden, frames):
    """every sent-mask is within its cap (none left out on `four`), every frame is recorded with its shape, is lit and fully weighted, traces at least its camera rays,
    and the media frames differ from the frame of the same scene without media"""
    for what, name in K.golden_pairs():
        key = "%d_%s" % (what, name)
        sent = golden[key + "_sent"]
        assert len(sent) == len(golden[key + "_q"]) == len(golden[key + "_out"]) >= K.GOLDEN_ROWS
        assert 1.0 - sent.mean() <= K.SENT_CAP, key
        assert sent.all() or (what in K.RULE_ONE and name != "four"), key
        assert golden[key + "_out"][sent.astype(bool)].any(), key
    assert {name for _, name in K.golden_pairs()} == set(K.GOLDEN_SETS) and {w for w, _ in K.golden_pairs()} == set(K.FUNCTIONS)
    assert all((w, "four") in K.golden_pairs() for w in K.RULE_ONE)
    generate = _generate()
    for case in generate.pathtrace_media_cases():
        key, make, w, h, direct, first = case
        rgb = frames[key + "_rgb"]
        assert rgb.shape == (h, w, 3) and frames[key + "_rays"].shape == (h, w), key
        assert frames[key + "_weight"].sum() > 0.9 * w * h * generate.MEDIA_PASSES and rgb.mean() > 1e-3, key
        assert int(frames[key + "_rays"].min()) >= 1, key
        if not key.startswith("clear"):
            clear = frames[generate.clear_case_of(case) + "_rgb"]
            assert np.abs(rgb - clear).mean() > 0.05 * clear.mean(), key
