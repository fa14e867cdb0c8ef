"""Key-mode serving (recommend.BatchPredict -> goctr_batch_predict -> serve_score_keys) OFF the shapes every other serving test
builds: tests/test_gpu_rank.py's build() with default arguments is cosine attention, hidden widths 200 / 80, Ip = 32, 48 or 144
and an embedding width of 4, 8, 12, 16 (DIN) or 64 (YouTube).  Here: the attention variants, input widths, hidden widths, embedding
widths and history lengths at which the host (csrc/serve.hip serve_score_keys; csrc/ctr.hip attn_fast_mode, serve16_ok,
launch_serve16, launch_attn_fwd, chain_ok, launch_chain, launch_forward) picks another kernel or another instantiation.

Every case: about 700 keys on 40 users and 300 items with an unknown user and an embedding-only item (two failed keys), a
maxTs == 0 key, a user whose history was emptied, an item without an embedding.  Scores within ctr_ref.LOGIT_TOL (1e-5) of the
oracle's composition of the same steps AND of its float64 evaluation of the same assembled rows; bit-equal over every path the
shape has (one launch / key lookup inside attn_fwd / rows assembled first) and over the one-launch pass's ways of waiting.  A second
test asserts, from the host's own report (goctr_prof_*: a serving slot's launches are counted and their symbols noted, not timed),
that each path ran the kernel the case is here for.

The host's arithmetic.  I = U + 2 D + Cc, Ip = I rounded up to 16; L = D / 4 lanes per embedding row; F = 1 YouTube, 2 DIN cosine,
3 DIN Euclidean.  fuse (key lookup inside the attention): D a multiple of 4 with L a power of two <= 16, i.e. D = 4 .. 64; every
other width assembles the rows first (assemble_keys_kernel) and runs attn_fwd_kernel<4,32 or 64,0> (D % 4 == 0),
attn_fwd_kernel<1,8 .. 64,0> or attn_fwd_wide_kernel<2 or 4> (scalar lanes).  chain_ok: H1p / 16 = 13 or 14, H2p = 80, Ip <= 240,
DIN: Dp <= 32 -- else the three layers are generic GEMM launches (gemm_fwd0 / gemm_fwd1 / gemm_out) on the serving slot's
workspace.  One launch (ctr_serve16_kernel<L,F,H>): fuse, L = 2, 4 or 16, chain_ok, fewer than 32 x CUs rows; H = 10 h0 fragments in
registers up to Ip = 160, else 15.  Otherwise attn_fwd_keys_kernel<L,F> and, with chain_ok, ctr_fwd16_kernel<4,5>, which takes
80 columns of h0 per K phase: one phase up to Ip = 80, two up to 160, three from 176.

  euclid-D4 / D8 / D16 / D32, euclid-D8-T70    DIN att = 1, (U, Cc) = (7, 9): keys<1,3> + fwd16; serve16<2,3,10>; serve16<4,3,10>;
                                               keys<8,3> + fwd16; T = 70 with histories up to 400: two id blocks, the bisection
  youtube-D4 / D8 / D16 / D32                  keys<1,1> + fwd16; serve16<2,1,10>; serve16<4,1,10>; keys<8,1> + fwd16
  cos-D32                                      keys<8,2> + fwd16: no D = 32 pass of any kind ran before
  din-D64-cos / -eucl                          Dp = 64 > 32: no chain for DIN -> keys<16,2> / <16,3> + the generic GEMMs (Ip = 144)
  ip80 / ip96 / ip160 / ip176 / ip240 / ip256  DIN cosine D = 16, (U, Cc) = (20, 28) I = 80: one full phase, no pad column;
                                               (30, 30) I = 92: two phases; (60, 68) I = 160: the last H = 10; (60, 70) I = 162 -> 176:
                                               the first H = 15, three phases; (100, 108) I = 240: 15 fragments (the model also
                                               holds bf16-split images, which a small pass does not use); (110, 110) I = 252 -> 256
                                               > 240: generic GEMMs behind keys<4,2>
  youtube-D64-ip192                            (30, 30), I = 188: serve16<16,1,15>
  h224x80 / h220x70 / h195x66, youtube-h220x70 (7, 9), D = 16: 14 tiles of H1 split 4,4,3,3 over the wavefronts; pad columns of H1
                                               and H2 inside serve16 / fwd16 (masked by n < H1, n < H2)
  x3-h195x66                                   (52, 53): Ip = 144, H1p = 208: bf16-split images with pad columns (the large pass below)
  h304x96 / h50x7, din and youtube             keys<4,F> + launch_nn on the slot's workspace (allocated because !chain_ok)
  asm-D6 / D70 / D100 / D128 / D256,           rows assembled first: attn_fwd_kernel<1,8,0>, attn_fwd_wide_kernel<2>,
  asm-D100-eucl, asm-youtube-D100              attn_fwd_kernel<4,32,0> (25 lanes; 32 lanes: a power of two, but > 16), <4,64,0>;
                                               DIN: generic GEMMs but for D = 6 (Dp = 16: fwd16); YouTube D = 100: I = 216 -> 224,
                                               fwd16 with three phases behind assembled rows
  T1 / T64 / T65 / T130 x hist30 / hist400     DIN cosine D = 16: the window edges of the key lookup, one / two / three 64-slot id
                                               blocks, ballot search / bisection

Large passes (32 x CUs rows and 17 more; CUs from goctr_device_info): no one-launch pass, and launch_chain leaves fwd16 for
ctr_chain_x3_kernel<9,true> (one 32-row tile per CU) / ctr_fwd4_kernel<9,false> (more tiles than CUs) where the model has
bf16-split images, else ctr_chain_kernel<7,5,0> run forward only; 304 / 96: the persistent generic GEMM.  And one request of
65 536 + 300 keys through the C-ABI, which serve_keys_direct cuts into two passes."""
import ctypes as C
import functools
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ctr_ref import LOGIT_TOL  # noqa: E402
from test_gpu_rank import build, oracle_rows, oracle_scores  # noqa: E402

pytestmark = pytest.mark.gpu

FWD16 = "ctr_fwd16_kernel<4,5>"
GENERIC = None                      # no chain launch: gemm_fwd0 / gemm_fwd1 / gemm_out, one launch each


def case(cid, kind, D, one, keys, asm, chain, att=0, T=10, max_hist=30, U=7, Cc=9, hidden=None):
    """one: ctr_serve16_kernel's symbol or None (the shape has no one-launch pass); keys: attn_fwd_keys_kernel's symbol or None (the
    rows are always assembled first); asm: the attention symbol behind assembled rows; chain: the chain symbol of a pass that is
    not one launch, or GENERIC"""
    return types.SimpleNamespace(id=cid, kind=kind, att=att, D=D, T=T, max_hist=max_hist, U=U, Cc=Cc, hidden=hidden, one=one, keys=keys,
                                 asm=asm, chain=chain)


def s16(L, F, H):
    return f"ctr_serve16_kernel<{L},{F},{H}>"


def keysk(L, F):
    return f"attn_fwd_keys_kernel<{L},{F}>"


def fast(L, F):
    return f"attn_fwd_kernel<4,{L},{F}>"


CASES = [
    # Euclidean attention in serving
    case("euclid-D4", 0, 4, None, keysk(1, 3), fast(1, 3), FWD16, att=1),
    case("euclid-D8", 0, 8, s16(2, 3, 10), keysk(2, 3), fast(2, 3), FWD16, att=1),
    case("euclid-D16", 0, 16, s16(4, 3, 10), keysk(4, 3), fast(4, 3), FWD16, att=1),
    case("euclid-D32", 0, 32, None, keysk(8, 3), fast(8, 3), FWD16, att=1),
    case("euclid-D8-T70", 0, 8, s16(2, 3, 10), keysk(2, 3), fast(2, 3), FWD16, att=1, T=70, max_hist=400),
    # YouTube below D = 64
    case("youtube-D4", 1, 4, None, keysk(1, 1), fast(1, 1), FWD16),
    case("youtube-D8", 1, 8, s16(2, 1, 10), keysk(2, 1), fast(2, 1), FWD16),
    case("youtube-D16", 1, 16, s16(4, 1, 10), keysk(4, 1), fast(4, 1), FWD16),
    case("youtube-D32", 1, 32, None, keysk(8, 1), fast(8, 1), FWD16),
    case("cos-D32", 0, 32, None, keysk(8, 2), fast(8, 2), FWD16),
    # DIN at D = 64: no chain
    case("din-D64-cos", 0, 64, None, keysk(16, 2), fast(16, 2), GENERIC),
    case("din-D64-eucl", 0, 64, None, keysk(16, 3), fast(16, 3), GENERIC, att=1),
    # the input width
    case("ip80", 0, 16, s16(4, 2, 10), keysk(4, 2), fast(4, 2), FWD16, U=20, Cc=28),
    case("ip96", 0, 16, s16(4, 2, 10), keysk(4, 2), fast(4, 2), FWD16, U=30, Cc=30),
    case("ip160", 0, 16, s16(4, 2, 10), keysk(4, 2), fast(4, 2), FWD16, U=60, Cc=68),
    case("ip176", 0, 16, s16(4, 2, 15), keysk(4, 2), fast(4, 2), FWD16, U=60, Cc=70),
    case("ip240", 0, 16, s16(4, 2, 15), keysk(4, 2), fast(4, 2), FWD16, U=100, Cc=108),
    case("ip256", 0, 16, None, keysk(4, 2), fast(4, 2), GENERIC, U=110, Cc=110),
    case("youtube-D64-ip192", 1, 64, s16(16, 1, 15), keysk(16, 1), fast(16, 1), FWD16, U=30, Cc=30),
    # hidden widths the chain accepts
    case("h224x80", 0, 16, s16(4, 2, 10), keysk(4, 2), fast(4, 2), FWD16, hidden=(224, 80)),
    case("h220x70", 0, 16, s16(4, 2, 10), keysk(4, 2), fast(4, 2), FWD16, hidden=(220, 70)),
    case("h195x66", 0, 16, s16(4, 2, 10), keysk(4, 2), fast(4, 2), FWD16, hidden=(195, 66)),
    case("youtube-h220x70", 1, 16, s16(4, 1, 10), keysk(4, 1), fast(4, 1), FWD16, hidden=(220, 70)),
    case("x3-h195x66", 0, 16, s16(4, 2, 10), keysk(4, 2), fast(4, 2), FWD16, U=52, Cc=53, hidden=(195, 66)),
    # hidden widths it refuses
    case("din-h304x96", 0, 16, None, keysk(4, 2), fast(4, 2), GENERIC, hidden=(304, 96)),
    case("youtube-h304x96", 1, 16, None, keysk(4, 1), fast(4, 1), GENERIC, hidden=(304, 96)),
    case("din-h50x7", 0, 16, None, keysk(4, 2), fast(4, 2), GENERIC, hidden=(50, 7)),
    case("youtube-h50x7", 1, 16, None, keysk(4, 1), fast(4, 1), GENERIC, hidden=(50, 7)),
    # embedding widths without a key variant: rows assembled first
    case("asm-D6", 0, 6, None, None, "attn_fwd_kernel<1,8,0>", FWD16),
    case("asm-D70", 0, 70, None, None, "attn_fwd_wide_kernel<2>", GENERIC),
    case("asm-D100", 0, 100, None, None, "attn_fwd_kernel<4,32,0>", GENERIC),
    case("asm-D128", 0, 128, None, None, "attn_fwd_kernel<4,32,0>", GENERIC),
    case("asm-D256", 0, 256, None, None, "attn_fwd_kernel<4,64,0>", GENERIC),
    case("asm-D100-eucl", 0, 100, None, None, "attn_fwd_kernel<4,32,0>", GENERIC, att=1),
    case("asm-youtube-D100", 1, 100, None, None, "attn_fwd_kernel<4,32,0>", FWD16),
] + [
    # the behaviour window
    case(f"T{T}-hist{h}", 0, 16, s16(4, 2, 10), keysk(4, 2), fast(4, 2), FWD16, T=T, max_hist=h)
    for T in (1, 64, 65, 130) for h in (30, 400)
]
N_KEYS = 700


def plant_keys(gr, rng, rs, uids, iids, extra, n):
    """n keys with the planted ones: (keys, number of failing keys)"""
    keys = [gr.Sample(int(rng.choice(uids)), int(rng.choice(iids)), 0.0, int(rng.integers(0, 1100))) for _ in range(n)]
    keys[3] = gr.Sample(4242, keys[3].ItemId, 0.0, 50)                 # unknown user: zero row, failed
    keys[10] = gr.Sample(keys[10].UserId, extra[0], 0.0, 50)           # embedding-only item: zero row, failed
    keys[11] = gr.Sample(keys[11].UserId, keys[11].ItemId, 0.0, 0)     # maxTs == 0: from the newest
    keys[20] = gr.Sample(uids[1], keys[20].ItemId, 0.0, 700)           # a user with an empty history
    keys[21] = gr.Sample(uids[1], iids[-1], 0.0, 0)                    # ... and an item without an embedding (iids[-15:] lack one)
    keys[22] = gr.Sample(keys[22].UserId, iids[-2], 0.0, 900)
    return keys, 2


@functools.lru_cache(maxsize=None)
def fixture(cid):
    """a case's recsys, model pair, keys and the oracle's two answers, computed once and left unchanged"""
    from goctr_amd import recommend as gr
    from oracle import pyoracle as oracle
    oracle.lib()
    c = next(c for c in CASES if c.id == cid)
    rng = np.random.default_rng(4000 + CASES.index(c))
    rs, om, net, uids, iids, extra = build(oracle, rng, c.kind, T=c.T, D=c.D, U=c.U, Cc=c.Cc, max_hist=c.max_hist, att=c.att, hidden=c.hidden)
    rs.DeleteUserBehavior([uids[1]])
    assert len(rs._dense_cache.ub[uids[1]].Ts) == 0
    keys, n_failed = plant_keys(gr, rng, rs, uids, iids, extra, N_KEYS)
    X, failed = oracle_rows(oracle, rs, *rs.keys(keys))
    assert not X[21, c.U + c.T * c.D:c.U + c.T * c.D + c.D].any() and not X[20, c.U:c.U + c.T * c.D].any()
    ref = om.predict(X, 256)
    ref64 = om.loss_grad_f64(X, np.zeros(len(keys)))[2]
    return types.SimpleNamespace(case=c, rs=rs, om=om, net=net, keys=keys, n_failed=n_failed, failed=failed, ref=ref, ref64=ref64,
                                 model=gr.Predictor(rs, net, predBatchSize=256))


PATHS = (("1", "1"), ("1", "0"), ("0", "1"))          # (GOCTR_SERVE_FUSE, GOCTR_SERVE_ONE_LAUNCH): one launch / keys / assembled


@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_scores_against_oracle_and_float64_on_every_path(monkeypatch, cid):
    from goctr_amd import recommend as gr
    f = fixture(cid)
    c = f.case
    ys = []
    for fuse, one in PATHS:
        monkeypatch.setenv("GOCTR_SERVE_FUSE", fuse)
        monkeypatch.setenv("GOCTR_SERVE_ONE_LAUNCH", one)
        ys.append(gr.BatchPredict(f.model, f.keys)[:, 0].copy())
    d32, d64 = float(np.max(np.abs(ys[0] - f.ref))), float(np.max(np.abs(ys[0] - f.ref64)))
    print(f"\ncase {cid}: device - oracle {d32:.2e}  device - float64 {d64:.2e}  (oracle - float64 {np.max(np.abs(f.ref - f.ref64)):.2e})")
    assert f.failed.sum() == f.n_failed == 2
    assert ys[0].shape == (N_KEYS,) and np.all(np.isfinite(ys[0]))
    assert d32 <= LOGIT_TOL
    assert d64 <= LOGIT_TOL
    assert np.array_equal(ys[0], ys[1]) and np.array_equal(ys[0], ys[2])
    # failing keys score exactly as the all-zero row does
    zero = f.om.predict(np.zeros((1, f.om.xcols), np.float32), 1)[0]
    assert np.all(np.abs(ys[0][f.failed.astype(bool)] - zero) <= LOGIT_TOL)
    if c.one is None:
        return
    # the one-launch pass with the host waiting on the stream / watching the workgroups' stamps whatever the pass size, and with
    # the kernels reading the keys from the pinned host buffer instead of over the PCIe BAR
    monkeypatch.setenv("GOCTR_SERVE_FUSE", "1")
    monkeypatch.setenv("GOCTR_SERVE_ONE_LAUNCH", "1")
    for rows in ("0", "100000"):
        monkeypatch.setenv("GOCTR_SERVE_POLL_ROWS", rows)
        for _ in range(2):                               # (stamps are pass numbers: consecutive passes must not see old ones)
            assert np.array_equal(gr.BatchPredict(f.model, f.keys)[:, 0], ys[0]), rows
    monkeypatch.delenv("GOCTR_SERVE_POLL_ROWS")
    monkeypatch.setenv("GOCTR_SERVE_BAR", "0")
    assert np.array_equal(gr.BatchPredict(f.model, f.keys)[:, 0], ys[0])


def profiled(fn):
    """(launch counts by family, symbols by family) of fn()'s launches; fn's result"""
    from goctr_amd import capi
    capi.prof_enable(True)
    try:
        capi.prof_reset()
        out = fn()
        n = {k: v[1] for k, v in capi.prof_get().items()}
        syms = capi.prof_kernels()
    finally:
        capi.prof_enable(False)
    return n, syms, out


def check_layers(n, syms, chain):
    if chain is GENERIC:
        assert n["chain"] == 0 and n["gemm_fwd0"] == 1 and n["gemm_fwd1"] == 1 and n["gemm_out"] == 1
    else:
        assert n["chain"] == 1 and syms["chain"] == chain
        assert n["gemm_fwd0"] == 0 and n["gemm_fwd1"] == 0 and n["gemm_out"] == 0


@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_the_case_runs_the_kernels_it_is_here_for(monkeypatch, cid):
    """so that a later change of the dispatch cannot silently empty a case: what the host reports for one 700-row pass on each
    path -- one launch: no attention launch, the chain family's one launch is ctr_serve16_kernel<L,F,H>; else the attention symbol
    (key variant or the assembled rows' kernel) and the chain symbol or the three generic GEMM launches.  The profiled passes return
    the unprofiled passes' bits."""
    from goctr_amd import recommend as gr
    f = fixture(cid)
    c = f.case
    got = []
    for (fuse, one), path in zip(PATHS, ("one", "keys", "asm")):
        monkeypatch.setenv("GOCTR_SERVE_FUSE", fuse)
        monkeypatch.setenv("GOCTR_SERVE_ONE_LAUNCH", one)
        n, syms, y = profiled(lambda: gr.BatchPredict(f.model, f.keys)[:, 0].copy())
        got.append(y)
        if path == "one" and c.one is not None:
            assert n["attn_fwd"] == 0 and n["chain"] == 1 and syms["chain"] == c.one, (n, syms)
            assert n["gemm_fwd0"] == 0 and n["gemm_out"] == 0
            continue
        want_attn = c.asm if (path == "asm" or c.keys is None) else c.keys
        assert n["attn_fwd"] == 1 and syms["attn_fwd"] == want_attn, (path, n, syms)
        check_layers(n, syms, c.chain)
    monkeypatch.delenv("GOCTR_SERVE_FUSE")
    monkeypatch.delenv("GOCTR_SERVE_ONE_LAUNCH")
    want = gr.BatchPredict(f.model, f.keys)[:, 0]
    assert all(np.array_equal(y, want) for y in got)


# ---------------------------------------------------------------------------------------------------------------------
# large passes

# (U, Cc, hidden, chain symbol at 32 x CUs rows, at 17 more); D = 16, DIN cosine, T = 10
LARGE = [
    ("x3-200x80", 52, 53, None, "ctr_chain_x3_kernel<9,true>", "ctr_fwd4_kernel<9,false>"),
    ("200x80", 7, 9, None, "ctr_chain_kernel<7,5,0>", "ctr_chain_kernel<7,5,0>"),
    ("220x70", 7, 9, (220, 70), "ctr_chain_kernel<7,5,0>", "ctr_chain_kernel<7,5,0>"),
    ("304x96", 7, 9, (304, 96), GENERIC, GENERIC),
    # beyond the issue's four: the forward-only bf16-split kernels with pad columns in H1 and H2 (they had only run 200 / 80)
    ("x3-195x66", 52, 53, (195, 66), "ctr_chain_x3_kernel<9,true>", "ctr_fwd4_kernel<9,false>"),
]


@pytest.mark.parametrize("name,U,Cc,hidden,sym_even,sym_more", LARGE, ids=[p[0] for p in LARGE])
def test_passes_of_a_32_row_tile_per_compute_unit_and_more(oracle, monkeypatch, name, U, Cc, hidden, sym_even, sym_more):
    """N = 32 x CUs and N + 17 keys in one pass: serve16_ok is false and launch_chain leaves the 16-row forward kernel (the
    module's docstring); against the oracle, bit-equal with the rows assembled first, and the symbols the host reports"""
    from goctr_amd import capi, recommend as gr
    rng = np.random.default_rng(4500 + len(name))
    rs, om, net, uids, iids, extra = build(oracle, rng, 0, U=U, Cc=Cc, hidden=hidden)
    cus = capi.device_info()[1]
    assert cus > 0
    rs.DeleteUserBehavior([uids[1]])
    model = gr.Predictor(rs, net, predBatchSize=4096)
    n_more = 32 * cus + 17
    keys, n_failed = plant_keys(gr, rng, rs, uids, iids, extra, n_more)
    ref, failed = oracle_scores(oracle, rs, om, keys, 4096)
    assert failed.sum() == n_failed
    for n, sym in ((32 * cus, sym_even), (n_more, sym_more)):
        cnt, syms, y = profiled(lambda: gr.BatchPredict(model, keys[:n])[:, 0].copy())
        assert cnt["attn_fwd"] == 1 and syms["attn_fwd"] == "attn_fwd_keys_kernel<4,2>", (cnt, syms)
        check_layers(cnt, syms, sym)
        print(f"\nlarge pass {name} n = {n}: device - oracle {np.max(np.abs(y - ref[:n])):.2e}")
        assert np.max(np.abs(y - ref[:n])) <= LOGIT_TOL
        assert np.array_equal(gr.BatchPredict(model, keys[:n])[:, 0], y)
        monkeypatch.setenv("GOCTR_SERVE_FUSE", "0")
        assert np.array_equal(gr.BatchPredict(model, keys[:n])[:, 0], y)
        monkeypatch.delenv("GOCTR_SERVE_FUSE")


def test_a_request_of_more_rows_than_one_pass_holds(oracle):
    """65 536 + 300 keys (7, 9, D 8, T 5) through goctr_batch_predict with numpy key arrays: serve_keys_direct scores them as two
    passes on one slot; every row against the oracle, and the bits of two calls on the two halves.  Ip = 32 has bf16-split images, so
    the full pass is ctr_fwd4_kernel<2,false> -- and so must the 300-row tail be (StepOpts::dispatch_rows): left to its own row
    count it took ctr_serve16_kernel<2,2,10>, whose scores differ in the last bit (one of the 65 836 was an ulp off the halves')"""
    from goctr_amd import capi
    rng = np.random.default_rng(4600)
    rs, om, net, uids, iids, extra = build(oracle, rng, 0, T=5, D=8)
    n = 65536 + 300
    users = rng.integers(0, rs.user_table.shape[0], size=n).astype(np.int32)
    items = rng.integers(0, rs.item_table.shape[0], size=n).astype(np.int32)
    ts = rng.integers(0, 1100, size=n).astype(np.int64)
    users[5] = rs.user_table.shape[0] + 3                                    # unknown user
    items[9] = rs.item_table.shape[0] + 2                                    # an item beyond the feature table
    users[65536 + 7] = -1                                                    # ... and one failing key in the second pass
    ts[11] = 0

    def call(lo, hi):
        y, failed, nf = np.full(hi - lo, np.nan, np.float32), np.zeros(hi - lo, np.uint8), C.c_int64(0)
        capi.check(capi.load().goctr_batch_predict(net._h, rs._h, capi.ptr(users[lo:hi], C.c_int32), capi.ptr(items[lo:hi], C.c_int32),
                                                   capi.ptr(ts[lo:hi], C.c_int64), C.c_int64(hi - lo), C.c_int(4096), capi.ptr(y, C.c_float),
                                                   capi.ptr(failed, C.c_uint8), C.byref(nf)))
        return y, failed, nf.value

    y, failed, nf = call(0, n)
    X, ref_failed = oracle_rows(oracle, rs, users, items, ts)
    ref = om.predict(X, 4096)
    assert nf == 3 and np.array_equal(failed, ref_failed) and ref_failed.sum() == 3
    print(f"\n{n} keys: device - oracle {np.max(np.abs(y - ref)):.2e}")
    assert np.max(np.abs(y - ref)) <= LOGIT_TOL
    half = n // 2
    (ya, fa, na), (yb, fb, nb) = call(0, half), call(half, n)
    assert np.array_equal(np.concatenate([ya, yb]), y) and np.array_equal(np.concatenate([fa, fb]), failed) and na + nb == 3
    # two passes, and the second one's kernels are the first one's
    cnt, syms, (yp, _, _) = profiled(lambda: call(0, n))
    assert cnt["attn_fwd"] == 2 and cnt["chain"] == 2 and syms["chain"] == "ctr_fwd4_kernel<2,false>", (cnt, syms)
    assert np.array_equal(yp, y)
    # ... while the same 300 keys as a request of their own are one launch
    cnt, syms, _ = profiled(lambda: call(65536, n))
    assert cnt["attn_fwd"] == 0 and cnt["chain"] == 1 and syms["chain"] == "ctr_serve16_kernel<2,2,10>", (cnt, syms)
