"""CPU checks around the ranks of given targets: the NumPy restatement (tests/rankutil.py) against np.argsort(kind="stable") and
over shards, utils.retrieval.ranks_from_counts / recall_from_counts (pure host arithmetic) against it, the ABI's two entry points and
their host-side refusals, the --eval-recall flag and retrieve.py's --recall arguments.  No GPU.
Integers are compared exactly; the float64 metrics within relative 1e-12 (means of at most a few dozen terms in another order)."""
import os
import re
import subprocess

import numpy as np
import pytest

import rankutil as U
from conftest import ROOT

RTOL = 1e-12


@pytest.mark.parametrize("bits", [16, 33, 64])
@pytest.mark.parametrize("zeros", [False, True])
def test_index_rank_is_the_position_in_a_stable_argsort(bits, zeros):
    qB, rB = U.codes(9, 301, bits, zeros, 100 + bits)
    h = U.half_units(qB, rB)
    assert h.min() >= 0 and h.max() <= 2 * bits and (zeros == bool((h % 2).any()))
    t = U.targets(9, 301, 4, 7, pad=False)
    c = U.counts(h, t)
    order = np.argsort(h, axis=1, kind="stable")
    where = np.empty_like(order)
    np.put_along_axis(where, order, np.arange(301)[None, :].repeat(9, 0), 1)          # where[q, j] = the column of item j
    np.testing.assert_array_equal(U.ranks(c, "index"), np.take_along_axis(where, t, 1))
    assert (c[..., 2] >= 1).all() and (c[..., 1] < c[..., 2]).all() and (c[..., 2] > 1).any()
    assert (U.ranks(c, "optimistic") <= U.ranks(c, "index")).all() and (U.ranks(c, "index") <= U.ranks(c, "pessimistic")).all()
    np.testing.assert_array_equal(2 * U.ranks(c, "expected"), U.ranks(c, "optimistic") + U.ranks(c, "pessimistic"))


@pytest.mark.parametrize("step", [100, 64, 1])
def test_shard_counts_with_clamped_bounds_add_up(step):
    qB, rB = U.codes(7, 257, 16, True, 5)
    h = U.half_units(qB, rB)
    t = U.targets(7, 257, 5, 11)
    t[2, 3], t[3, 1], t[4, 2] = step - 1, step, 256 - 256 % step        # last of a shard, first of the next, first of the last one
    total = sum(U.counts(h, t, a, min(257, a + step)) for a in range(0, 257, step))
    np.testing.assert_array_equal(total, U.counts(h, t))
    assert (total[t < 0] == 0).all() and (total[t >= 0][:, 2] > 0).all()


def _cases():
    """counts [Q, G, 3] by hand and from codes: G = 1, G = 5 with padding in every slot, a query without a target."""
    out = {}
    for name, (Q, n, K, G, seed) in {"g1": (12, 90, 16, 1, 1), "g5": (13, 90, 16, 5, 2)}.items():
        qB, rB = U.codes(Q, n, K, False, seed)
        t = U.targets(Q, n, G, seed + 50)
        out[name] = U.counts(U.half_units(qB, rB), t)
    assert (out["g5"][-1] == 0).all() and (out["g5"][..., 2] == 0).any(0).all()      # an empty row; padding in every slot position
    out["none"] = np.zeros((3, 2, 3), np.int64)
    # ties = 1 (the target alone at its distance) and ties > K at K = 5: less = 3 -> in; less = 7 -> out; less = 2, ties = 9 -> 3 / 9
    out["expected"] = np.array([[[3, 0, 1]], [[7, 0, 1]], [[2, 4, 9]], [[0, 0, 40]], [[5, 0, 2]]], np.int64)
    return out


@pytest.mark.parametrize("name", ["g1", "g5", "none", "expected"])
def test_functions_on_cpu_tensors_equal_the_restatement(name):
    import torch
    import cmh_native as N
    import utils.retrieval as R
    c = _cases()[name]
    ct = torch.from_numpy(c)
    ks = (1, 5, 10)
    for ties in U.TIES:
        got = R.ranks_from_counts(ct, ties)
        want = U.ranks(c, ties)
        assert got.dtype == (torch.float64 if ties == "expected" else torch.int64) and not got.is_cuda
        np.testing.assert_array_equal(got.numpy(), want)                    # (NaN == NaN here)
        m, w = R.recall_from_counts(ct, ks, ties), U.metrics(c, ks, ties)
        assert isinstance(m, dict) and m["recall"].dtype == torch.float64 and m["recall"].shape == (3,)
        np.testing.assert_allclose(m["recall"].numpy(), w["recall"], rtol=RTOL, atol=0)
        np.testing.assert_allclose([m["median_rank"], m["mean_rank"]], [w["median_rank"], w["mean_rank"]], rtol=RTOL, atol=0)
        np.testing.assert_array_equal(m["best_rank"].numpy(), w["best_rank"])
        if ties == "expected":
            assert "mrr" not in m
            with pytest.raises(N.NativeError):
                m["mrr"]
        else:
            np.testing.assert_allclose(m["mrr"], w["mrr"], rtol=RTOL, atol=0)
    int32 = R.recall_from_counts(ct.to(torch.int32), ks, "index")           # the native call's dtype
    np.testing.assert_array_equal(int32["recall"].numpy(), R.recall_from_counts(ct, ks, "index")["recall"].numpy())
    if name == "expected":
        e = R.recall_from_counts(ct, (5,), "expected")
        np.testing.assert_allclose(e["recall"].numpy(), [(1 + 0 + 3 / 9 + 5 / 40 + 0) / 5], rtol=RTOL, atol=0)
        np.testing.assert_array_equal(e["best_rank"].numpy(), [4.0, 8.0, 7.0, 20.5, 6.5])
    if name == "none":
        assert R.recall_from_counts(ct, ks, "index")["best_rank"].tolist() == [-1, -1, -1]
    with pytest.raises(ValueError):
        R.ranks_from_counts(ct, "random")
    with pytest.raises(ValueError):
        R.recall_from_counts(ct, (0, 5))
    with pytest.raises(ValueError):
        R.recall_from_counts(ct[:, :, :2])


def test_abi_carries_both_names():
    import cmh_native as N
    lib = N.lib()
    names = {"cmh_rank_workspace_bytes", "cmh_hamming_rank"}
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cmh.h")).read(), flags=re.S)
    assert names <= set(re.findall(r"\b(cmh_[a-z0-9_]+)\s*\(", header))
    assert names <= set(N.SIGNATURES)
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    assert names <= set(re.findall(r" T (cmh_[a-z0-9_]+)", out))
    assert lib.cmh_version() == N.ABI_VERSION == 6                    # entry points were added, nothing else changed
    assert len(N.SIGNATURES["cmh_hamming_rank"][1]) == 15 and len(N.SIGNATURES["cmh_rank_workspace_bytes"][1]) == 4


def test_workspace_query_answers_without_a_gpu():
    import cmh_native as N
    lib = N.lib()
    for Q, n, bits, G in ((1, 1, 1, 1), (9, 1000, 16, 8), (130, 1031, 64, 5), (65, 1031, 128, 1), (64, 1031, 160, 2),
                          (65535, 524287, 2048, 8), (5000, 190834, 128, 1)):
        got = lib.cmh_rank_workspace_bytes(Q, n, bits, G)
        assert got >= Q * G * 4 + 3 * G * 256 * ((Q + 63) // 64), (Q, n, bits, G)      # the targets' distances and one image per tile
        assert got < 64 << 20                                                           # no columns: small whatever the shape
    for Q, n, bits, G in ((0, 10, 16, 1), (65536, 10, 16, 1), (10, 0, 16, 1), (10, 524288, 16, 1), (10, 10, 0, 1), (10, 10, 2049, 1),
                          (-1, 10, 16, 1), (10, 10, 16, 0), (10, 10, 16, 9), (10, 10, 16, -1)):
        assert lib.cmh_rank_workspace_bytes(Q, n, bits, G) == 0, (Q, n, bits, G)


def test_native_refusals_come_before_any_launch():
    """Null operands, G outside 1..8, sizes outside the limits and a short workspace return a negative status with a message:
    nothing is launched, so this runs without a GPU.  (Non-null pointers are host addresses the call never reads.)"""
    import ctypes as C
    import cmh_native as N
    lib = N.lib()
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    big = 1 << 40

    def call(qs=p, qn=p, rs=p, rn=p, Q=4, n=10, bits=16, ts=p, tn=p, bound=p, G=2, out=p, ws=p, ws_bytes=big):
        return lib.cmh_hamming_rank(qs, qn, rs, rn, Q, n, bits, ts, tn, bound, G, out, ws, ws_bytes, None)

    bad = [dict(qs=None), dict(qn=None), dict(rs=None), dict(rn=None), dict(ts=None), dict(tn=None), dict(bound=None), dict(out=None),
           dict(G=0), dict(G=9), dict(G=-3), dict(Q=0), dict(Q=65536), dict(n=0), dict(n=524288), dict(bits=0), dict(bits=2049),
           dict(ws=None), dict(ws_bytes=0), dict(ws_bytes=lib.cmh_rank_workspace_bytes(4, 10, 16, 2) - 1)]
    for kw in bad:
        assert call(**kw) < 0, kw
        assert len(lib.cmh_last_error()) > 0


def test_binding_and_functions_refuse_bad_arguments_on_the_host():
    import torch
    import cmh_native as N
    import utils.retrieval as R
    planes = (torch.zeros(2, 1, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32))
    with pytest.raises(N.NativeError):                                # CPU tensors: no fallback
        N.hamming_rank(planes, planes, 16, planes, torch.zeros(2, 1, dtype=torch.int32))
    codes = torch.ones(2, 16)
    bad = [torch.tensor([0.0, 1.0]), torch.tensor([0, 2]), torch.tensor([0, -2]), torch.tensor([0, 1, 1]), torch.zeros(2, 0, dtype=torch.int64),
           torch.tensor([True, False])]
    for targets in bad:                                               # (without a GPU the functions refuse before they look)
        with pytest.raises(N.NativeError):
            R.target_counts(codes, codes, targets)
        with pytest.raises(N.NativeError):
            R.recall_at_k(codes, codes, targets)
    with pytest.raises(N.NativeError):
        R.recall_at_k(torch.ones(3, 16), codes)                       # identity pairing: more queries than items
    with pytest.raises((ValueError, N.NativeError)):
        R.recall_at_k(codes, codes, ties="random")


def test_eval_recall_flag_is_off_by_default():
    import argsbase
    assert argsbase.get_baseargs().parse_known_args([])[0].eval_recall is False
    args = argsbase.get_baseargs().parse_known_args(["--eval-recall", "true"])[0]
    assert args.eval_recall is True and args.eval_graded is False and args.eval_curves is False


def test_retrieve_recall_arguments():
    import retrieve
    a = retrieve.parse(["--codes", "x.mat", "--recall"])
    assert a.recall and a.ks == [1, 5, 10] and a.ties == "index" and a.targets is None and a.k is None
    a = retrieve.parse(["--codes", "x.mat", "--recall", "--ks", "1,50", "--ties", "expected", "--index", "db.npz", "--targets", "t.txt",
                        "--queries", "0:3", "--direction", "t2i"])
    assert a.ks == [1, 50] and a.ties == "expected" and a.targets == "t.txt" and a.index == "db.npz"
    a = retrieve.parse(["--codes", "x.mat", "--k", "3"])
    assert not a.recall and a.ks is None and a.ties is None and a.targets is None
    refused = [["--recall", "--radius", "1"], ["--recall", "--map"], ["--recall", "--graded"], ["--recall", "--k", "3"],
               ["--recall", "--index", "db.npz"],                      # --index needs --targets
               ["--recall", "--ks", "0,5"], ["--recall", "--ks", "a"], ["--recall", "--ks", ""], ["--recall", "--ties", "random"],
               ["--ks", "1,5"], ["--ties", "index"], ["--targets", "t.txt"], ["--k", "3", "--ties", "expected"]]
    for extra in refused:
        with pytest.raises(SystemExit) as e:
            retrieve.parse(["--codes", "x.mat"] + extra)
        assert e.value.code != 0, extra
