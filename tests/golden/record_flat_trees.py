"""Records tests/golden/flat_trees.json, the trees tests/test_flat_tree_golden.py holds the flattener to.

The trees come from the library of the PARENT of the commit that changes the builder, never from the code under test: build that parent in a scratch worktree
(python -m cudatracerlib_amd.build there), then, in this tree,

    CTL_AMD_LIB=<parent>/cudatracerlib_amd/libctl_amd.so python tests/golden/record_flat_trees.py <parent>/cudatracerlib_amd/libctl_knobs.so

The cases and the hashing are the test module's own."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.environ.get("CTL_AMD_LIB"):
        sys.exit(__doc__)
    import test_flat_tree_golden as t
    from cudatracerlib_amd import api
    api.set_cache_dir(None)
    out = {name: t.records_of(name) for name in t.SCENES}
    for knob in t.KNOBS:
        out[knob] = t.knob_records(knob, os.path.abspath(sys.argv[1]))
    with open(t.GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    for k, v in out.items():
        print(k, {f: (r["n_nodes"], r["n_leaves"], r["n_part_boxes"]) for f, r in v.items()})
