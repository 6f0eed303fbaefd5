"""Host side of the soft queries' mAP by counting, without a GPU: the float64 restatement of tests/softaputil.py against
mapcountutil's where the two must agree, the rules it moves with, what the generated cases hold, the refusals of cmh_soft_ap and of
the Python layers that need no GPU, and auc_from_rank_sum on cases worked out by hand."""
import math
import os
import re

import numpy as np
import pytest
import torch

import mapcountutil as mu
import softaputil as su
import softutil
from conftest import ROOT


def test_entry_points_in_binding_and_header():
    import cmh_native as N
    header = open(os.path.join(ROOT, "include", "cmh.h")).read()
    for name in ("cmh_soft_ap_workspace_bytes", "cmh_soft_ap"):
        assert name in N.SIGNATURES and re.search(r"\b%s\s*\(" % name, header)
    assert N.ABI_VERSION == 6


def test_restatement_on_a_case_by_hand():
    """One query with weights (15, -8): items and their wdist 23 - r . w; relevant = items 1, 2, 4."""
    u = np.array([[1.0, -8 / 15]], np.float32)
    rB = np.array([[1, -1], [1, 1], [-1, 1], [0, 0], [1, 1], [-1, -1]], np.float32)
    w, _, _ = softutil.quantise(u)
    assert w.tolist() == [[15, -8]]
    assert softutil.wdist(w, rB).tolist() == [[0, 16, 46, 23, 16, 30]]
    qL = np.array([[1, 0]], np.float32)
    rL = np.array([[0, 1], [1, 0], [1, 1], [0, 1], [1, 0], [0, 0]], np.float32)
    # order: 0 (0), 1 (16), 4 (16), 3 (23), 5 (30), 2 (46): the relevant items 1, 4, 2 have ranks 2, 3, 6
    ap, R, rank_sum = su.restated(u, rB, qL, rL, (None, 1, 2, 6))
    assert R.tolist() == [3] and rank_sum.tolist() == [11]
    assert ap[None][0] == (1 / 2 + 2 / 3 + 3 / 6) / 3 and ap[6][0] == ap[None][0]
    assert ap[1][0] == 1 / 2 and ap[2][0] == (1 / 2 + 2 / 3) / 2


@pytest.mark.parametrize("zeros", [False, True])
def test_saturated_queries_reproduce_the_binary_restatement(zeros):
    """u = c * (a code without zeros): every weight is +-15, wdist = 15 h, so R, the ranks and the APs are mapcountutil's."""
    qB, rB, qL, rL = mu.case(9, 700, 32, False, 24)[0], mu.case(9, 700, 32, zeros, 24)[1], *mu.case(9, 700, 32, zeros, 24)[2:]
    u = (qB * np.float32(0.37)).astype(np.float32)
    w, _, _ = softutil.quantise(u)
    assert (np.abs(w) == 15).all() and np.array_equal(softutil.wdist(w, rB), 15 * mu.half_units(qB, rB))
    ks = (None, 1, 5, 50)
    ap, R, _ = su.restated(u, rB, qL, rL, ks)
    want = mu.restated_ap(qB, rB, qL, rL, ks)
    assert np.array_equal(R, mu.relevance(qL, rL).sum(1))
    for k in ks:
        assert np.array_equal(ap[k], want[k][0]), k


def test_restatement_moves_when_a_rule_is_broken():
    u, rB, qL, rL = su.case(9, 700, 16, True, 24, "coarse")
    ks = (None, 5)
    ap, R, rank_sum = su.restated(u, rB, qL, rL, ks)
    # ties by `>`: equal distances in descending index order
    ap_t, R_t, rank_sum_t = su.restated(u, rB, qL, rL, ks, ties="reverse")
    assert np.array_equal(R, R_t) and not np.array_equal(rank_sum, rank_sum_t) and np.abs(ap[None] - ap_t[None]).max() > 1e-3
    # relrank <= total dropped: every relevant item adds a term although k = 5 admits five
    ap_a = su.restated(u, rB, qL, rL, ks, keep_all=True)[0]
    assert np.array_equal(ap[None], ap_a[None]) and np.abs(ap[5] - ap_a[5]).max() > 1e-3
    # k ignored
    ap_k = su.restated(u, rB, qL, rL, ks, use_k=False)[0]
    assert np.array_equal(ap_k[5], ap[None]) and np.abs(ap[5] - ap_k[5]).max() > 1e-3


@pytest.mark.parametrize("shape", [(5, 257, 16, True, 1, "coarse"), (5, 1025, 64, True, 24, "tanh"), (9, 700, 16, True, 24, "coarse"),
                                   (3, 4200, 128, True, 80, "tanh"), (65, 2049, 33, False, 33, "tanh")])
def test_cases_hold_what_they_claim(shape):
    u, rB, qL, rL = su.case(*shape)
    mu.check_label_mix(qL, rL)
    su.check_mix(u, rB, qL, rL)
    if shape[3]:
        assert (rB == 0).any()
    if shape[5] == "coarse":
        w = softutil.quantise(u)[0]
        assert (np.abs(w[1:, 1:]) <= 1).all() and (w[1:, 0] == 15).all()
    ks = su.k_values(qL, rL)
    R = mu.relevance(qL, rL).sum(1)
    assert ks[0] is None and 1 in ks and rL.shape[0] in ks and any(k is not None and k > R[R < rL.shape[0]].max() for k in ks)


def test_mean_in_query_order():
    ap = np.array([0.1, 0.7, 0.2, 0.9, 0.3], np.float32)
    acc = np.float32(0)
    for v in ap:
        acc = np.float32(acc + v)
    assert su.mean_f32(ap) == np.float32(acc / np.float32(5))


def test_abi_refusals_before_any_launch():
    """Nothing is launched: the checks run before any HIP call, so they answer without a GPU.  Every refusal names the call."""
    import cmh_native as N
    lib = N.lib()
    one, big = 16, 1 << 40

    def call(Q=1, n=100, bits=16, k=5, LW=1, ptrs=None, ws=one, nbytes=big):
        p = [one] * 9 if ptrs is None else ptrs
        return lib.cmh_soft_ap(p[0], p[1], p[2], p[3], p[4], p[5], LW, Q, n, bits, k, p[6], p[7], p[8], ws, nbytes, None)

    for kw, what in ((dict(Q=65), b"Q=65"), (dict(Q=0), b"Q=0"), (dict(bits=129), b"bits=129"), (dict(bits=0), b"bits=0"),
                     (dict(n=0), b"N=0"), (dict(n=2 ** 31), b"N=2147483648"), (dict(k=101), b"k=101"), (dict(k=-1), b"k=-1"),
                     (dict(LW=0), b"label_words=0")):
        assert call(**kw) == -1, kw
        assert what in lib.cmh_last_error() and b"soft_ap" in lib.cmh_last_error(), lib.cmh_last_error()
    for null in range(9):
        assert call(ptrs=[None if i == null else one for i in range(9)]) == -1
        assert b"soft_ap: null pointer" in lib.cmh_last_error()
    assert call(bits=64, ptrs=[16, 16, 20, 16, 16, 16, 16, 16, 16]) == -1 and b"aligned" in lib.cmh_last_error()     # rows of 8 bytes at 20
    assert call(bits=128, ptrs=[16, 16, 16, 24, 16, 16, 16, 16, 16]) == -1 and b"aligned" in lib.cmh_last_error()    # rows of 16 bytes at 24
    assert call(ptrs=[16, 16, 16, 16, 16, 16, 16, 16, 20]) == -1 and b"rank_sum" in lib.cmh_last_error()
    need = lib.cmh_soft_ap_workspace_bytes(1, 100, 16, 1)
    assert need > 0
    assert call(nbytes=need - 1) == -2 and b"soft_ap: workspace" in lib.cmh_last_error()
    assert call(ws=None, nbytes=need) == -2
    # k = 0 means N, k = N is legal: both reach the workspace check
    assert call(k=0, nbytes=0) == -2 and call(k=100, nbytes=0) == -2


def test_workspace_query_and_its_limits():
    import cmh_native as N
    lib = N.lib()
    for Q, n, bits, LW in ((0, 10, 16, 1), (65, 10, 16, 1), (1, 0, 16, 1), (1, 2 ** 31, 16, 1), (1, 10, 0, 1), (1, 10, 129, 1), (1, 10, 16, 0)):
        assert lib.cmh_soft_ap_workspace_bytes(Q, n, bits, LW) == 0, (Q, n, bits, LW)
    # the images stay under 256 MiB; beside them 33 words per (row, bin), 16 bytes per (chunk, query) and 8 bytes per item
    for Q in (1, 3, 17, 64):
        for n in (1, 4099, 2_000_000, 2 ** 31 - 1):
            for bits in (1, 64, 128):
                got = lib.cmh_soft_ap_workspace_bytes(Q, n, bits, 3)
                assert 8 * n < got <= (256 << 20) + 2 * Q * (30 * bits + 1) * 33 * 4 + 8 * n + (4 << 20), (Q, n, bits, got)


def test_python_refusals_before_the_gpu():
    """By name, from CPU tensors, before anything is packed: they hold with and without a GPU."""
    import cmh_native as N
    import utils.retrieval as R
    u, rB = torch.zeros(3, 16), torch.ones(10, 16)
    qL, rL = torch.ones(3, 4), torch.ones(10, 4)
    with pytest.raises(N.NativeError, match="soft_mean_average_precision: labels on one side only"):
        R.soft_mean_average_precision(u, rB, qL, None)
    with pytest.raises(N.NativeError, match="soft_mean_average_precision: needs the labels of both sides"):
        R.soft_mean_average_precision(u, rB, None, None)
    with pytest.raises(N.NativeError, match="soft_topk: labels on one side only"):
        R.soft_topk(u, rB, 5, query_L=qL)
    with pytest.raises(N.NativeError, match="soft_topn_precision: labels on one side only"):
        R.soft_topn_precision(u, rB, None, rL)
    with pytest.raises(N.NativeError, match="soft_mean_average_precision: 12-entry soft queries for codes of 16 bits"):
        R.soft_mean_average_precision(torch.zeros(3, 12), rB, qL, rL)
    bad = u.clone()
    bad[1, 3] = float("nan")
    with pytest.raises(N.NativeError, match="soft_mean_average_precision: a soft query must be finite"):
        R.soft_mean_average_precision(bad, rB, qL, rL)
    bad[1, 3] = float("inf")
    with pytest.raises(N.NativeError, match="soft_topk: a soft query must be finite"):
        R.soft_topk(bad, rB, 5, query_L=qL, retrieval_L=rL)
    with pytest.raises(N.NativeError, match="bits=160 exceeds 128"):
        R.soft_mean_average_precision(torch.zeros(3, 160), torch.ones(10, 160), qL, rL)
    with pytest.raises(N.NativeError, match="labels of 2 queries for 3 soft queries"):
        R.soft_mean_average_precision(u, rB, qL[:2], rL)
    with pytest.raises(N.NativeError, match="soft_ap: needs the labels of both sides"):
        N.soft_ap((None, None), (None, None), 16, None, None)


def test_cpu_only_call_is_refused_by_name(monkeypatch):
    import cmh_native as N
    import utils.retrieval as R
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)      # (a machine without a GPU, wherever this runs)
    with pytest.raises(N.NativeError, match="needs a GPU"):
        R.soft_mean_average_precision(torch.zeros(3, 16), torch.ones(10, 16), torch.ones(3, 4), torch.ones(10, 4))
    z = torch.zeros(1, 1, dtype=torch.int32)
    with pytest.raises(N.NativeError, match="GPU only"):
        N.soft_ap((z, z.view(1, 1, 1).expand(1, 4, 1).contiguous()), (z, z), 16, z, z)


def test_auc_from_rank_sum_by_hand():
    from utils.retrieval import auc_from_rank_sum
    # n = 5: relevant at ranks 1, 2: perfect; at 4, 5: worst; at 2, 4: U = 6 - 3 = 3 of 6 pairs wrong
    auc = auc_from_rank_sum(torch.tensor([3, 9, 6]), torch.tensor([2, 2, 2]), 5)
    assert auc.dtype == torch.float64 and auc.tolist() == [1.0, 0.0, 0.5]
    # R = 0 and R = n: no pair to order
    auc = auc_from_rank_sum([0, 15], [0, 5], 5)
    assert all(math.isnan(v) for v in auc.tolist())
    # one relevant item at rank r among n: AUC = 1 - (r - 1) / (n - 1); integers beyond 2^53 stay exact before the division
    n = 2 ** 31 - 1
    assert auc_from_rank_sum([1, n, 2], [1, 1, 1], n).tolist() == [1.0, 0.0, 1.0 - 1 / (n - 1)]
    R = 2 ** 30
    best = R * (R + 1) // 2
    assert auc_from_rank_sum(torch.tensor([best, best + R * (n - R)]), torch.tensor([R, R], dtype=torch.int32), n).tolist() == [1.0, 0.0]
    # equal to the pair count of the definition on a random ranking
    rng = np.random.default_rng(3)
    rel = rng.random(200) < 0.3
    ranks = np.nonzero(rel)[0] + 1
    wrong = sum(int((~rel[:r - 1]).sum()) for r in ranks)
    got = auc_from_rank_sum([int(ranks.sum())], [int(rel.sum())], 200)[0].item()
    assert got == 1.0 - wrong / (int(rel.sum()) * int((~rel).sum()))
    with pytest.raises(ValueError, match="is not the rank sum"):
        auc_from_rank_sum([2], [2], 5)
    with pytest.raises(ValueError, match="rank sums for"):
        auc_from_rank_sum([2, 3], [2], 5)


def test_eval_soft_flag():
    import argsbase
    parser = argsbase.get_baseargs()
    assert parser.parse_args([]).eval_soft is False
    assert parser.parse_args(["--eval-soft", "true"]).eval_soft is True


def _gather_worker(rank, world, port, out_dir):
    from conftest import PKG  # noqa: F401  (puts the package on sys.path)
    import dist_utils as du
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    du.init_from_env("gloo")
    n, K = 37, 16                                          # ragged: the ranks encode 19 and 18 rows, in shuffled positions
    g = torch.Generator().manual_seed(0)
    img, txt = torch.tanh(torch.randn(n, K, generator=g)), torch.tanh(torch.randn(n, 2 * K, generator=g))
    img[3, 5], txt[7, 1] = 1e-30, -0.0                     # values no packed code could carry
    order = torch.randperm(n, generator=g)
    lo, hi = du.shard_range(n, rank, world)
    mine = order[lo:hi]
    a, b = torch.full((n, K), float("nan")), torch.full((n, 2 * K), float("nan"))
    a[mine], b[mine] = img[mine], txt[mine]
    du.gather_float_rows(mine, a, b)
    assert torch.equal(a.view(torch.int32), img.view(torch.int32)) and torch.equal(b.view(torch.int32), txt.view(torch.int32))
    # a rank without rows still takes part
    c = torch.zeros(n, K)
    if rank == 0:
        c[:] = img
    du.gather_float_rows(torch.arange(n) if rank == 0 else torch.empty(0, dtype=torch.int64), c)
    assert torch.equal(c, img)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()
    open(os.path.join(out_dir, f"sg{rank}"), "w").write("ok")


def test_world2_gloo_gather_of_soft_rows(tmp_path):
    """The trainers' exchange of soft query rows between processes (dist_utils.gather_float_rows): bit for bit, positions included."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_gather_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert (tmp_path / "sg0").exists() and (tmp_path / "sg1").exists()
    # one process: nothing to do, nothing touched
    import dist_utils as du
    a = torch.ones(3, 2)
    du.gather_float_rows(torch.arange(3), a)
    assert torch.equal(a, torch.ones(3, 2))


@pytest.mark.parametrize("method", ["MITH", "TwDH"])
def test_methods_without_a_soft_rule_refuse_the_flag(method, tmp_path, monkeypatch):
    """By name, before a dataset is built, a model loaded or anything encoded: it needs no GPU."""
    import argparse
    import sys
    import main
    from code_rules import SOFT_RULES
    assert method not in SOFT_RULES
    monkeypatch.setattr(sys, "argv", ["main.py", "--save-dir", str(tmp_path), "--eval-soft", "true", "--pretrained", "none.pth"])
    with pytest.raises(ValueError, match=f"--eval-soft: method {method} has no soft rule"):
        main.trainers[method](argparse.Namespace(method=method, dataset="synthetic", output_dim=16, is_train=False), 0)
