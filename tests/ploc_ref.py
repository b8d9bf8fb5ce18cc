"""An independent restatement, in numpy, of stages 5 - 7 of the PLOC rebuild (csrc/flat_ploc.h, csrc/flat_rebuild.h): the clustering rounds, the 4-wide collapse
and the level-by-level layout, from what stages 1 - 4 hand over (FlatBvh.rebuild_order: the sorted order and the entries' boxes).  It shares no code with the library:
the rounds are vectorised over all clusters at once (the library's host twin walks them one by one, the device runs one lane each), the areas are float32 in the
library's expression order ((dx dy + dy dz) + dz dx), and the collapse works on plain Python lists.  tests/test_flat_ploc_host.py holds the host twin to it word for
word; the device is held to the host twin (tests/test_gpu_flat_ploc.py).

    tree = build(sorted_entry, entry_boxes, bounds)
    tree["mask"], tree["w10"], tree["w11"]   per node: the mask byte (word 3 >> 24) and the two link words
    tree["level_start"], tree["depth"]
    tree["perm"], tree["last"]               per new entry position: the entry it holds (index before the rebuild) and whether it closes its leaf
    tree["rounds"]
"""
import numpy as np

RADIUS = 8
LEAF_MAX = 4
f32 = np.float32


def cluster_boxes(sorted_entry, entry_boxes, bounds):
    B = entry_boxes[sorted_entry].astype(f32)
    inverted = ~((B[:, 0] <= B[:, 3]) & (B[:, 1] <= B[:, 4]) & (B[:, 2] <= B[:, 5]))
    B[inverted] = np.concatenate([bounds[3:], bounds[3:]])
    return B[:, :3].copy(), B[:, 3:].copy()


def union_area(lo_a, hi_a, lo_b, hi_b):
    d = (np.maximum(hi_a, hi_b) - np.minimum(lo_a, lo_b)).astype(f32)
    xy = (d[:, 0] * d[:, 1]).astype(f32); yz = (d[:, 1] * d[:, 2]).astype(f32); zx = (d[:, 2] * d[:, 0]).astype(f32)
    return ((xy + yz).astype(f32) + zx).astype(f32)


def cluster(lo, hi, radius=RADIUS):
    """the binary tree: left, right, count per inner node (id n + j), and the number of rounds"""
    n = len(lo)
    ids = np.arange(n, dtype=np.int64)
    left, right, count = np.zeros(max(n - 1, 0), np.int64), np.zeros(max(n - 1, 0), np.int64), np.zeros(max(n - 1, 0), np.int64)
    entries = lambda i: np.where(i < n, 1, count[np.maximum(i - n, 0)])
    made = rounds = 0
    while len(ids) > 1:
        m = len(ids); rounds += 1
        pos = np.arange(m)
        best = np.full(m, -1, np.int64); best_area = np.full(m, np.inf, f32)
        for off in list(range(-radius, 0)) + list(range(1, radius + 1)):        # smallest (area, i xor j) wins
            j = pos + off
            ok = (j >= 0) & (j < m)
            jj = np.clip(j, 0, m - 1)
            a = union_area(lo, hi, lo[jj], hi[jj])
            take = ok & ((best < 0) | (a < best_area) | ((a == best_area) & ((pos ^ jj) < (pos ^ np.maximum(best, 0)))))
            best[take] = j[take]; best_area[take] = a[take]
        mutual = best[best] == pos
        keep_merged = mutual & (pos < best)
        removed = mutual & (pos > best)
        k = int(keep_merged.sum())
        assert k > 0, "a round without a merge"
        rank = np.cumsum(keep_merged) - keep_merged
        a, b = ids[keep_merged], ids[best[keep_merged]]
        new = made + rank[keep_merged]
        left[new] = a; right[new] = b; count[new] = entries(a) + entries(b)
        nlo, nhi, nid = lo.copy(), hi.copy(), ids.copy()
        p = best[keep_merged]
        nlo[keep_merged] = np.minimum(lo[keep_merged], lo[p]); nhi[keep_merged] = np.maximum(hi[keep_merged], hi[p]); nid[keep_merged] = n + new
        lo, hi, ids = nlo[~removed], nhi[~removed], nid[~removed]
        made += k
    assert made == max(n - 1, 0)
    return left, right, count, rounds


def build(sorted_entry, entry_boxes, bounds, radius=RADIUS):
    n = len(sorted_entry)
    lo, hi = cluster_boxes(sorted_entry, entry_boxes, bounds)
    left, right, count, rounds = cluster(lo, hi, radius)
    left, right, count = left.tolist(), right.tolist(), count.tolist()
    size = lambda i: 1 if i < n else count[i - n]

    def entries_under(i):
        return [i] if i < n else entries_under(left[i - n]) + entries_under(right[i - n])

    def slots_of(node):
        S = [node]
        if size(node) <= LEAF_MAX:
            return S
        split = lambda k: S.__setitem__(slice(k, k + 1), [left[S[k] - n], right[S[k] - n]])
        split(0)
        if size(S[1]) > LEAF_MAX:
            split(1)
        if size(S[0]) > LEAF_MAX:
            split(0)
        while len(S) < 4:
            sizes = [size(x) for x in S]
            if max(sizes) <= LEAF_MAX:
                break
            split(sizes.index(max(sizes)))                                   # the lower slot on a tie
        return S

    root = 2 * n - 2 if n > 1 else 0
    level, level_start = [root], [0]
    mask, w10, w11, perm, last = [], [], [], [], []
    n_nodes_so_far, entry = 1, 0
    while level:
        nxt = []
        for node in level:
            S = slots_of(node)
            first_child, first_entry = n_nodes_so_far + len(nxt), entry
            mk, t, ni, nl = 0, [0, 0, 0, 0], 0, 0
            for k, x in enumerate(S):
                mk |= 1 << k
                if size(x) <= LEAF_MAX:
                    mk |= 16 << k; t[k] = 15 - nl; nl += size(x)
                    E = entries_under(x)
                    perm += [int(sorted_entry[e]) for e in E]; last += [False] * (len(E) - 1) + [True]; entry += len(E)
                else:
                    t[k] = ni << 2; ni += 1; nxt.append(x)
            if ni == 0:
                for k in range(len(S), 4):
                    mk |= 16 << k; t[k] = 15
            inner_base4 = first_child * 4 if ni else 0
            leaf_base = first_entry if nl else 0
            mask.append(mk)
            w10.append((inner_base4 | (t[1] << 26) | ((t[3] & 3) << 30)) & 0xffffffff)
            w11.append(((t[3] >> 2) | (t[2] << 2) | ((~(leaf_base + 15)) << 6)) & 0xffffffff)
        level_start.append(n_nodes_so_far)   # the end of this level
        n_nodes_so_far += len(nxt)
        level = nxt
    assert entry == n
    return dict(mask=np.array(mask, np.uint32), w10=np.array(w10, np.uint32), w11=np.array(w11, np.uint32), level_start=np.array(level_start, np.uint32),
                depth=len(level_start) - 2, perm=np.array(perm, np.uint32), last=np.array(last, bool), rounds=rounds)
