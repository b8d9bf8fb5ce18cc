"""Cases shared by tests/test_flat_ploc_host.py and tests/test_gpu_flat_ploc.py: the PLOC builder of the rebuild (csrc/flat_ploc.h).  Every case and pose of
tests/flat_rebuild_cases.py, and

SAME   one single-triangle mesh instanced nine times under ONE transform, over a floor quad: the nine boxes are equal, so every distance among them ties and only the
       tie rule (csrc/flat_ploc.h "Progress") decides whether a round merges anything, and how many rounds the nine take.  The smallest input at which it does.
"""
import numpy as np

from cudatracerlib_amd import api, scenes
import flat_rebuild_cases as frc

POSES = dict(frc.POSES, SAME=(None, "MV"))
CASES = [(c, p) for c, poses in POSES.items() for p in poses]
IDS = ["%s-%s" % (c, p or "built") for c, p in CASES]
REF_CASES = [(c, p) for c in ("T1", "T4", "T5", "TW", "SAME", "S3") for p in POSES[c]]            # held to tests/ploc_ref.py, node for node
QUALITY_CASES = [(c, p) for c in ("S1", "S2", "S3", "S3D3", "BIG") for p in POSES[c]]           # where PLOC has to beat the LBVH's node area
N_SAME = 9


def _same(pose, width, height):
    sc = api.DynamicScene()
    P, I, N = scenes._quad([[-6, 0, -6], [-6, 0, 6], [6, 0, 6], [6, 0, -6]], [0, 1, 0])
    sc.CreateNode(sc.add_mesh(P, I, normals=N, materials=[api.diffuse((0.6, 0.6, 0.6))]))
    tri = sc.add_mesh(np.array([[0, 0, 0], [1, 0, 0.2], [0.3, 1, 0]], np.float32), np.array([[0, 1, 2]], np.uint32), materials=[api.diffuse((0.3, 0.5, 0.7), two_sided=True)])
    xf = np.eye(4, dtype=np.float32); xf[:3, :3] *= 2.5; xf[:3, 3] = (-1.0, 1.5, 0.5)
    nodes = [sc.CreateNode(tri, xf) for _ in range(N_SAME)]
    if pose:
        xf = xf.copy(); xf[:3, 3] = (1.5, 2.5, -1.0); xf[1, 1] = 3.1
        for k in nodes:
            sc.SetNodeTransform(k, xf)
    sc.CreatePointLight((0, 9, -4), (60, 60, 60))
    sc.setCamera((0, 4, -11.5), (0, 2, 0), (0, 1, 0), 60.0, width, height)
    sc.UpdateScene()
    return sc


def new_scene(case, pose=None, width=32, height=32):
    return _same(pose, width, height) if case == "SAME" else frc.new_scene(case, pose, width, height)


def old_scene(case, width=32, height=32):
    return _same(None, width, height) if case == "SAME" else frc.old_scene(case, width, height)
