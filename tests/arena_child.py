"""The child process of tests/test_gpu_arena_poison.py's other arena routes:  python tests/arena_child.py OUT.json
It runs under the GOCTR_ARENA_MB its parent set -- 0: no arena, every buffer a hipMalloc and every release a hipFree; 1: a 1 MiB
arena, so that some buffers lie inside it and the larger ones outside -- and makes arena_cases.CHILD_CASES' calls: the recall-entries
recording against tests/golden/recall_entries.json and the metrics cases against tests/golden/metrics_frozen.json, with the
assertions of their own test files.  What it found goes to OUT.json; the parent asserts on it."""
import json
import os
import sys
import traceback

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arena_cases as A  # noqa: E402


def main(out_path):
    arena = A.Arena()
    res = {"arena_mb": os.environ.get("GOCTR_ARENA_MB"), "failed": {}, "passed": []}
    try:
        res["fill"] = list(arena.fill(0))
    except arena.capi.GoctrError as e:
        res["fill_refused"] = str(e)
    res["before"] = arena.stats()
    for name in A.CHILD_CASES:
        try:
            A.CASES[name]()
            res["passed"].append(name)
        except Exception:                                    # (an assertion of the case, or an error of the library: nothing
            res["failed"][name] = traceback.format_exc()[-1500:]      # more runs on the device behind it)
            break
    res["after"] = arena.stats()
    with open(out_path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1])
