"""CPU checks of BPR training (include/goctr.h: "BPR"): the restatement tests/bpr_ref.py holds the consequences the header states,
and the header, the ctypes binding and the library agree on the two names and on goctr_bpr_cfg."""
import ctypes as C
import os
import subprocess
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import als_cases as K  # noqa: E402
import als_ref as A  # noqa: E402
import bpr_ref as B  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_epochs_split_byte_for_byte_and_the_auc_rises():
    g = K.scene("base")[1]
    Y0 = A.init_y(3, K.N_ITEMS, 8)
    X0 = np.zeros((g["n_users"], 8))
    kw = dict(batch=256, lr=0.05, lam=0.01, seed=9)
    both = B.fit(g, X0, Y0, epochs=2, **kw)
    one = B.fit(g, X0, Y0, epochs=1, **kw)
    two = B.fit(g, one["X"], one["Y"], epochs=1, first_epoch=1, **kw)
    assert both["X"].tobytes() == two["X"].tobytes() and both["Y"].tobytes() == two["Y"].tobytes()
    assert both["loss"].tolist() == [one["loss"][0], two["loss"][0]] and np.array_equal(both["triples"][1], two["triples"][0])
    auc = B.fit(g, X0, Y0, epochs=5, **kw)["auc"]
    assert (np.diff(auc) > 0).all() and auc[4] > 0.6                             # (the sampled pairs are ranked better every epoch)
    held = [set(g["uitems"][g["uoff"][u]:g["uoff"][u + 1]].tolist()) for u in range(g["n_users"])]
    assert all(i in held[u] and j not in held[u] and j != 79 for u, i, j in both["triples"][0].tolist())      # item 79 has no edge


def test_header_binding_and_library_agree(tmp_path):
    from goctr_amd import capi
    lib = capi.load()
    assert {"goctr_bpr_cfg_default", "goctr_bpr_fit"} <= set(capi.SYMBOLS) and hasattr(lib, "goctr_bpr_fit")
    (tmp_path / "t.c").write_text('#include <stdio.h>\n#include <stddef.h>\n#include "goctr.h"\n'
                                  'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(goctr_bpr_cfg), offsetof(goctr_bpr_cfg, lr), '
                                  'offsetof(goctr_bpr_cfg, neg_tries), offsetof(goctr_bpr_cfg, seed), offsetof(goctr_bpr_cfg, reserved)); return 0; }\n')
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()))
    c, T = capi.default_bpr_cfg(), capi.BprCfg
    assert got == [C.sizeof(T), T.lr.offset, T.neg_tries.offset, T.seed.offset, T.reserved.offset]
    assert (c.epochs, c.first_epoch, c.batch, c.lr, c.lambda_, c.neg_tries, c.neg_source, c.seed, c.reserved) == (10, 0, 65536, 0.05, 0.01, 8, 0, 0, 0)


def test_fit_bpr_fails_loudly_without_a_handle():
    from goctr_amd import capi, recall as gl
    h = gl.ALS.__new__(gl.ALS)
    h._h, h.graph = None, types.SimpleNamespace(_h=None, n_edges=4)
    with pytest.raises(capi.GoctrError):
        h.fit_bpr(epochs=1, neg_source="popular", triples=True)
    assert gl.make_bpr_cfg(**{"lambda": 0.5, "neg_source": "popular"}).lambda_ == 0.5
