"""The flattened BVH (csrc/flatten.cpp) held to recorded trees, bit for bit: the builder is deterministic (the tree does not depend on the thread count), so the sha256 of
every array a tree is made of can be committed.  tests/golden/flat_trees.json was recorded with tests/golden/record_flat_trees.py from the library of the commit BEFORE
flatten_scene was split into stages; a change that is meant to alter the trees re-records it with the library of its own parent and says so.  CPU only."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "flat_trees.json")
FORMATS = ("q4", "q8")


def one_triangle():
    import cudatracerlib_amd as ctl
    sc = ctl.DynamicScene()
    V = np.array([[-1, 0, 0], [1, 0.25, 0], [0, 1, 0.5]], np.float32)
    sc.CreateNode(sc.add_mesh(V, np.array([[0, 1, 2]], np.uint32), normals=np.tile(np.float32([0, 0, 1]), (3, 1))))
    sc.setCamera((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0, 16, 16)
    sc.UpdateScene()
    return sc


def scene_of(name):
    from cudatracerlib_amd import scenes
    return {"sm_sub2": lambda: scenes.synthetic_sm(32, 32, n_instances=60, subdiv=2),
            "cornell_glass": lambda: scenes.cornell_box(32, 32, glass_sphere=True),
            "beams": lambda: scenes.beams_over_spheres(),              # 2582 split parts
            "one_triangle": one_triangle,                              # a single-node tree that carries a slab
            "fuzz3": lambda: scenes.fuzz_scene(3),
            "sm_sub4": lambda: scenes.synthetic_sm(32, 32, n_instances=60, subdiv=4)}[name]()   # ~307 k references: the BVH2 builder's threaded partition


SCENES = ("sm_sub2", "cornell_glass", "beams", "one_triangle", "fuzz3", "sm_sub4")
# builder options only the measurement build reads (csrc/knobs.h), once per process: each in a child process, on the first scene.  CTL_FLAT_BFS_TOP=64: with the
# default of 65 536 nodes a small tree is breadth-first throughout and the depth-first part of the memory order would not run
KNOBS = ("CTL_FLAT_FORCE_EXPLICIT=1", "CTL_FLAT_COLLAPSE=1", "CTL_FLAT_SLOT_ORDER=1", "CTL_FLAT_SPLIT=0", "CTL_FLAT_BFS_TOP=64")


def tree_record(fb):
    """what is recorded of a FlatBvh: the hash of each of its arrays and its scalars"""
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    idx, boxes = fb.parts()
    d = fb.desc
    return dict(format=int(d.format), n_nodes=int(d.n_nodes), n_leaves=int(d.n_leaves), max_depth=int(d.max_depth), compact=int(d.compact), root_slab=int(d.root_slab),
                n_slab_nodes=int(d.n_slab_nodes), n_part_boxes=int(d.n_part_boxes), nodes=sha(fb.nodes()), leaves=sha(fb.leaves()), child_links=sha(fb.child_links()),
                part_index=sha(idx) if idx is not None else None, part_boxes=sha(boxes) if boxes is not None else None)


def records_of(name):
    """{format name: record} of one scene, built by the library this process has loaded"""
    from cudatracerlib_amd import api
    sc = scene_of(name)
    return {f: tree_record(api.FlatBvh(sc.desc, api.FLAT_FORMATS[f])) for f in FORMATS}


def knob_records(knob, lib):
    """the first scene's records from a child process that loads `lib` with the knob set"""
    k, v = knob.split("=")
    code = "import sys, json; sys.path[:0] = [%r, %r]; import test_flat_tree_golden as t; print('RECORDS', json.dumps(t.records_of(%r)))" % (ROOT, os.path.join(ROOT, "tests"), SCENES[0])
    env = dict(os.environ, CTL_AMD_LIB=lib, **{k: v})
    env.pop("CTL_CACHE_DIR", None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RECORDS ")][-1][8:])


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(autouse=True)
def no_cache():
    from cudatracerlib_amd import api
    api.set_cache_dir(None)
    yield
    api.set_cache_dir(None)


@pytest.mark.parametrize("name", SCENES)
def test_tree_equals_the_recorded_one(golden, name):
    got = records_of(name)
    for f in FORMATS:
        assert got[f] == golden[name][f], (name, f)
    assert got["q4"]["format"] == 0 and got["q8"]["format"] == 3      # no recorded Q8 tree is the 4-wide fallback


@pytest.mark.parametrize("knob", KNOBS)
def test_knobs_build_equals_the_recorded_tree(golden, knob):
    got = knob_records(knob, os.path.join(ROOT, "cudatracerlib_amd", "libctl_knobs.so"))
    for f in FORMATS:
        assert got[f] == golden[knob][f], (knob, f)
    assert got["q4"] != golden[SCENES[0]]["q4"]                       # every one of these knobs changes the 4-wide tree


def test_cold_build_and_warm_load_equal_the_recorded_tree(golden, tmp_path):
    from cudatracerlib_amd import api
    api.set_cache_dir(str(tmp_path / "cache"))
    cold = records_of("beams")
    files = sorted(f for f in os.listdir(str(tmp_path / "cache")) if f.startswith("flat_"))
    assert len(files) == 2
    warm = records_of("beams")
    assert sorted(f for f in os.listdir(str(tmp_path / "cache")) if f.startswith("flat_")) == files
    assert cold == warm == golden["beams"]
