"""Volume sets and query rows of the participating-media tests (not collected): shared by tests/test_volume_host.py (ctl_volume_eval on the host against the
restatement) and tests/test_gpu_volume.py (the same queries on the device against the host).

SETS:  one      one volume over the Cornell box (HG 0.7, coloured sigma_s)
       half     one isotropic volume over the lower half of it: a ray that touches the box is scattered over its WHOLE segment (the reference's quirk)
       two      two overlapping volumes with different phase functions (Rayleigh; Kajiya-Kay under a rotation, whose WorldBound() is larger than the region)
       sixteen  a 4 x 4 grid of regions, all four phase functions, with the coefficient corner cases: sig_s = 0, sig_t = 0, one zero channel, a density whose
                transmittance falls under 1e-8, g = 0 and |g| = 0.9
       four     (GOLDEN_SETS only: the fixture recorded from the reference, tests/golden/volumes.npz) four regions laid out so that sampleVolume's index — ffsn's bit
                MASK, as written — stays inside the table for every ray: region 0 the Cornell box, region 1 a box around every ray origin, regions 2 and 3 two small
                cubes in opposite corners that no ray of the population crosses both.  The masks that occur are 2 (index 2), 3 (index 1), 7 and 11 (index 1 or 2)
queries(set, volumes, what, n): n seeded rows plus the branch points of that function."""
import numpy as np

from cudatracerlib_amd import api

f32 = np.float32
BOX_LO = np.array([0.0, 0.0, 0.0], np.float32)
BOX_HI = np.array([556.0, 548.8, 559.2], np.float32)
SETS = ("one", "half", "two", "sixteen")
GOLDEN_SETS = SETS + ("four",)
GOLDEN_ROWS = 256   # seeded rows per function and set in tests/golden/volumes.npz (plus the branch points)
FUNCTIONS = {api.VEVAL_REGION_INTERSECT: "region IntersectP", api.VEVAL_INTERSECT: "aggregate IntersectP", api.VEVAL_REGION_TAU: "region tau", api.VEVAL_TAU: "aggregate tau",
             api.VEVAL_REGION_SAMPLE_DISTANCE: "region sampleDistance", api.VEVAL_SAMPLE_DISTANCE: "aggregate sampleDistance", api.VEVAL_SAMPLE_VOLUME: "sampleVolume",
             api.VEVAL_PHASE_EVAL: "phase Evaluate", api.VEVAL_PHASE_SAMPLE: "phase Sample", api.VEVAL_P: "aggregate p", api.VEVAL_SAMPLE: "aggregate Sample",
             api.VEVAL_TRANSMITTANCE: "Transmittance", api.VEVAL_EVAL_TRANSMITTANCE: "evalTransmittance"}
_REGION = (api.VEVAL_REGION_INTERSECT, api.VEVAL_REGION_TAU, api.VEVAL_REGION_SAMPLE_DISTANCE, api.VEVAL_PHASE_EVAL, api.VEVAL_PHASE_SAMPLE)


def _rot_y(deg, scale, translate):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    m = np.array([[c * scale[0], 0, s * scale[2], translate[0]], [0, scale[1], 0, translate[1]], [-s * scale[0], 0, c * scale[2], translate[2]], [0, 0, 0, 1]], np.float32)
    return m


def make_set(name):
    box = api.box_to_volume_matrix
    if name == "one":
        return [api.homogeneous_volume(box(BOX_LO, BOX_HI), 0.0005, (0.002, 0.001, 0.003), api.phase_hg(0.7))]
    if name == "half":
        return [api.homogeneous_volume(box(BOX_LO, BOX_HI * np.array([1, 0.5, 1], np.float32)), 0.001, 0.004, api.phase_isotropic())]
    if name == "two":
        return [api.homogeneous_volume(box((0, 0, 0), (400, 548.8, 400)), (0.001, 0.0, 0.002), 0.002, api.phase_rayleigh()),
                api.homogeneous_volume(_rot_y(30.0, (300, 300, 300), (200, 100, 150)), 0.0005, (0.004, 0.002, 0.001), api.phase_kajiya_kay(0.4, 0.2, 4.0))]
    if name == "sixteen":
        phases = [api.phase_isotropic(), api.phase_hg(0.0), api.phase_hg(0.9), api.phase_hg(-0.9), api.phase_rayleigh(), api.phase_kajiya_kay(0.3, 0.5, 2.5)]
        coeff = [(0.002, 0.0), (0.0, 0.0), ((0.0, 0.001, 0.002), (0.0, 0.003, 0.001)), (0.5, 0.5), (0.0, 0.003), (0.001, (0.004, 0.0005, 0.002))]   # (sig_a, sig_s)
        out = []
        for k in range(16):
            i, j = k % 4, k // 4
            lo = np.array([i * 139.0, 0.0, j * 139.8], np.float32); hi = lo + np.array([160.0, 548.8 - 40.0 * (k % 3), 160.0], np.float32)   # neighbours overlap
            sa, ss = coeff[k % len(coeff)]
            out.append(api.homogeneous_volume(box(lo, hi), sa, ss, phases[(k * 5 + 1) % len(phases)]))
        return out
    if name == "four":
        return [api.homogeneous_volume(box(BOX_LO, BOX_HI), 0.0005, 0.002, api.phase_isotropic()),
                api.homogeneous_volume(box((-400, -400, -400), (1000, 1000, 1000)), (0.0002, 0.0004, 0.0001), (0.0006, 0.001, 0.0015), api.phase_hg(0.5)),
                api.homogeneous_volume(box((0, 0, 0), (160, 160, 160)), 0.001, (0.004, 0.002, 0.001), api.phase_rayleigh()),
                api.homogeneous_volume(box((396, 388.8, 0), (556, 548.8, 160)), 0.0005, 0.003, api.phase_kajiya_kay(0.4, 0.2, 4.0))]
    raise ValueError(name)


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def _idx(i):
    return np.array(i, np.uint32).view(np.float32)


def _sampling_weight(v):
    """m_mediumSamplingWeight of a region, in fp32 as sampleDistance derives it (only to aim a query just under it)"""
    with np.errstate(all="ignore"):
        sa, ss = np.array(list(v.sig_a), np.float32), np.array(list(v.sig_s), np.float32)
        st = sa + ss; al = ss / st
        w = f32(-1)
        for i in range(3):
            if al[i] > w and st[i] != 0:
                w = al[i]
        if w > 0:
            w = max(w, f32(0.5))
    return f32(w)


def queries(set_name, volumes, what, n):
    rs = np.random.RandomState(1000 + 17 * what + GOLDEN_SETS.index(set_name))
    nv = len(volumes)
    o = rs.uniform(-300, 900, (n, 3)).astype(np.float32)
    inside = rs.rand(n) < 0.5
    o[inside] = (BOX_LO + (BOX_HI - BOX_LO) * rs.rand(int(inside.sum()), 3)).astype(np.float32)   # half the rays start inside the box
    d = _unit(rs.normal(size=(n, 3)))
    minT = np.zeros(n, np.float32)
    maxT = np.where(rs.rand(n) < 0.3, f32(3.402823466e+38), rs.uniform(0, 1500, n)).astype(np.float32)
    smp = rs.rand(n).astype(np.float32)
    vi = rs.randint(0, nv, n)
    # branch points shared by the ray functions: a miss (pointing away), grazing rays in a face of the box (axis-parallel: 0 / 0 in the slab test), a start inside,
    # a start on a corner, a zero-length segment
    bo = [(-100, 300, 300), (278, 0, 100), (0, 100, 100), (278, 274, 280), (0, 0, 0), (278, 274, 280), (100, 100, -50), (556, 548.8, 559.2)]
    bd = [(-1, 0, 0), (1, 0, 0), (0, 0, 1), (0, 1, 0), _unit((1, 1, 1)), (0, 0, -1), (0, 0, 1), _unit((-1, -1, -1))]
    bmax = [3.402823466e+38, 3.402823466e+38, 1000, 50, 3.402823466e+38, 0, 40, 2000]
    nb = len(bo)
    o = np.concatenate([o, np.array(bo, np.float32)]); d = np.concatenate([d, np.array(bd, np.float32)])
    minT = np.concatenate([minT, np.zeros(nb, np.float32)]); maxT = np.concatenate([maxT, np.array(bmax, np.float32)])
    vi = np.concatenate([vi, np.arange(nb) % nv]); smp = np.concatenate([smp, rs.rand(nb).astype(np.float32)])
    N = len(o)
    q = np.zeros((N, 10), np.float32)
    if what in (api.VEVAL_REGION_INTERSECT, api.VEVAL_REGION_TAU, api.VEVAL_REGION_SAMPLE_DISTANCE):
        q[:, 0] = _idx(vi.astype(np.uint32)); q[:, 1:4] = o; q[:, 4:7] = d; q[:, 7] = minT; q[:, 8] = maxT; q[:, 9] = smp
    elif what in (api.VEVAL_INTERSECT, api.VEVAL_TAU, api.VEVAL_SAMPLE_DISTANCE, api.VEVAL_SAMPLE_VOLUME, api.VEVAL_TRANSMITTANCE):
        q[:, 0:3] = o; q[:, 3:6] = d; q[:, 6] = minT; q[:, 7] = maxT; q[:, 8] = smp
    elif what == api.VEVAL_EVAL_TRANSMITTANCE:
        q[:, 0:3] = o; q[:, 3:6] = (o + d * np.minimum(maxT, f32(1500))[:, None]).astype(np.float32)
    elif what in (api.VEVAL_PHASE_EVAL, api.VEVAL_PHASE_SAMPLE):
        wi = _unit(rs.normal(size=(N, 3))); wo = _unit(rs.normal(size=(N, 3)))
        q[:, 0] = _idx(vi.astype(np.uint32)); q[:, 1:4] = wi
        if what == api.VEVAL_PHASE_EVAL:
            q[:, 4:7] = wo
            q[-1, 1:4] = 0; q[-2, 1:4] = 0   # wi = 0 (Kajiya-Kay's early return)
            q[-3, 4:7] = q[-3, 1:4]; q[-4, 4:7] = -q[-4, 1:4]   # forward and backward
        else:
            q[:, 4:6] = rs.rand(N, 2).astype(np.float32)
            q[-1, 4:6] = (0, 0); q[-2, 4:6] = (np.nextafter(f32(1), f32(0)), np.nextafter(f32(1), f32(0))); q[-3, 4:6] = (0.5, 0.25)
        if nv > 1:   # every region's phase function sees the special rows
            extra = q[-4:].copy()
            rows = [extra.copy() for _ in range(nv)]
            for k, r in enumerate(rows):
                r[:, 0] = _idx(np.uint32(k))
            q = np.concatenate([q] + rows)
    elif what in (api.VEVAL_P, api.VEVAL_SAMPLE):
        wi = _unit(rs.normal(size=(N, 3)))
        q[:, 0:3] = o; q[:, 3:6] = wi
        if what == api.VEVAL_P:
            q[:, 6:9] = _unit(rs.normal(size=(N, 3)))
        else:
            q[:, 6:8] = rs.rand(N, 2).astype(np.float32)
    else:
        raise ValueError(what)
    if what in (api.VEVAL_REGION_SAMPLE_DISTANCE, api.VEVAL_SAMPLE_DISTANCE):
        # sample at 0, just under the sampling weight of each region, just under 1 — from a start inside the box along a long segment
        col = 9 if what == api.VEVAL_REGION_SAMPLE_DISTANCE else 8
        rows = []
        for k, v in enumerate(volumes):
            w = _sampling_weight(v)
            for s in (f32(0), np.nextafter(w, f32(0)) if w > 0 else f32(0.25), w if w > 0 else f32(0.75), np.nextafter(f32(1), f32(0)), f32(1e-7)):
                r = np.zeros(10, np.float32)
                if what == api.VEVAL_REGION_SAMPLE_DISTANCE:
                    r[0] = _idx(np.uint32(k)); r[1:4] = (278, 100, 280); r[4:7] = _unit((0.3, 0.1, 1)); r[7] = 0; r[8] = 900
                else:
                    r[0:3] = (278, 100, 280); r[3:6] = _unit((0.3, 0.1, 1)); r[6] = 0; r[7] = 900
                r[col] = s
                rows.append(r)
        q = np.concatenate([q, np.array(rows, np.float32)])
    return np.ascontiguousarray(q, np.float32)


def same_rows(got, want):
    """indices of the rows that differ: bit for bit where neither is a NaN, NaN for NaN"""
    got = np.asarray(got, np.float32); want = np.asarray(want, np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    ok = (gn & wn) | (~gn & ~wn & (got.view(np.uint32) == want.view(np.uint32)))
    return [int(i) for i in np.nonzero(~ok.all(axis=1))[0]]


# ---------------------------------------------------------------------------------------------------------------- the fixture recorded from the reference
RULE_ONE = (api.VEVAL_SAMPLE_DISTANCE, api.VEVAL_SAMPLE_VOLUME, api.VEVAL_SAMPLE)   # the functions that go through sampleVolume
SENT_CAP = 0.25   # at most this share of a function's rows on one set may be kept from the reference


def golden_pairs():
    """(function, set) pairs of tests/golden/volumes.npz: every function on every set, except the three functions that go through sampleVolume on `sixteen`, where the
    mask-as-index reads past the table in most rows (the set `four` stands in for it there)"""
    return [(what, name) for what in sorted(FUNCTIONS) for name in GOLDEN_SETS if not (name == "sixteen" and what in RULE_ONE)]


def sent_mask(V, what, q):
    """which query rows may be sent to the reference (1) — decided from the restatement V (volume_ref.Volumes) alone: a row in which sampleVolume forms an index past
    the table (the reference reads past m_pVolumes there; the product answers 'no region') is not sent.  Also returns the set of region masks that occurred."""
    sent = np.ones(len(q), np.uint8); masks = set()
    if what in RULE_ONE:
        for i, a in enumerate(np.asarray(q, np.float32).reshape(-1, 10)):
            if what == api.VEVAL_SAMPLE:
                raw = V.sample_volume_raw(a[0:3], a[3:6], f32(0), f32(3.402823466e+38), a[6])
            else:
                raw = V.sample_volume_raw(a[0:3], a[3:6], a[6], a[7], a[8])
            sent[i] = raw[0] < V.n; masks.add(int(raw[3]))
    return sent, masks


def table_digest(volumes):
    """sha256 over the ctl_volume array of a set, derived fields included"""
    import ctypes
    import hashlib
    return hashlib.sha256(b"".join(ctypes.string_at(ctypes.addressof(v), ctypes.sizeof(v)) for v in volumes)).hexdigest()


def with_normalization(volumes, values):
    """copies of the regions with Kajiya-Kay's m_normalization replaced by the given values (one per region; ignored for the other phase functions): the reference
    computes its own with glibc (tests/golden/volumes.npz records it), the product with the shared functions"""
    import ctypes
    out = []
    for v, n in zip(volumes, values):
        c = api.ctl_volume(); ctypes.memmove(ctypes.addressof(c), ctypes.addressof(v), ctypes.sizeof(c))
        if c.phase.type == api.PHASE_KAJIYA_KAY:
            c.phase.normalization = float(n)
        out.append(c)
    return out
