"""mAP, relevant counts and rank sums of soft queries by counting on the GPU (cmh_soft_ap, utils.retrieval.soft_mean_average_precision,
soft_topk with labels, soft_topn_precision, CodeIndex.map_soft, the trainers' --eval-soft) against the float64 restatement of
tests/softaputil.py.

Bounds.  relevant and rank_sum are integers: torch.equal.  AP and mAP: TOL_REF = 2.4e-7 of tests/test_gpu_map_count.py: the arithmetic
is the same (a term relrank / rank is one f32 quotient, <= 6e-8 relative, terms <= 1; the float64 sum of the terms is exact at
these sizes; the quotient by `total` is rounded to f32 once: two f32 ulps at 1), so the derivation there holds here."""
import numpy as np
import pytest
import torch

import mapcountutil as mu
import softaputil as su
import softutil

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_REF = 2.4e-7


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _near(tag, got_ap, want_ap, got_map=None):
    d_ap = float(np.abs(got_ap.cpu().numpy().astype(np.float64) - want_ap).max())
    d_map = 0.0 if got_map is None else abs(float(got_map) - float(want_ap.mean()))
    print(f"{tag}: max|ap - ref| = {d_ap:.3e}, |mAP - ref| = {d_map:.3e}")
    assert d_ap <= TOL_REF and d_map <= TOL_REF, (tag, d_ap, d_map)


def _check_case(Q, N, bits, zeros, C, style="tanh"):
    """soft_mean_average_precision == the restatement for every k of the case; -> the operands on the GPU."""
    from utils.retrieval import soft_mean_average_precision
    u, rB, qL, rL = su.case(Q, N, bits, zeros, C, style)
    want_ap, want_R, want_sum = su.case_reference(Q, N, bits, zeros, C, style)
    ops = [_t(x) for x in (u, rB, qL, rL)]
    for k, want in want_ap.items():
        mp, ap, relevant, rank_sum = soft_mean_average_precision(*ops, k=k, return_ap=True)
        assert mp.dtype == torch.float32 and mp.dim() == 0 and not mp.is_cuda
        assert ap.dtype == torch.float32 and relevant.dtype == torch.int32 and rank_sum.dtype == torch.int64
        assert ap.shape == relevant.shape == rank_sum.shape == (Q,)
        assert torch.equal(relevant.cpu(), torch.from_numpy(want_R).int()), (Q, N, bits, k)
        assert torch.equal(rank_sum.cpu(), torch.from_numpy(want_sum)), (Q, N, bits, k)
        _near(f"Q={Q} N={N} bits={bits} zeros={zeros} C={C} {style} k={k}", ap, want, mp)
        assert (ap[relevant == 0] == 0).all()
    return ops


@pytest.mark.parametrize("bits", [16, 20, 32, 33, 64, 96, 127, 128])
def test_code_widths_and_garbage_behind_the_last_bit(bits):
    """1..4 words per plane, widths that end inside a word; 2049 items: two chunks of the plan's minimum and a ragged third.  Then
    every bit at and behind `bits` set in both database planes and in q_mag: nothing of it may be counted."""
    import cmh_native as N
    Q, n, C = 5, 2049, 24
    ops = _check_case(Q, n, bits, True, C)
    su.check_mix(*su.case(Q, n, bits, True, C))
    if bits % 32:
        want_ap, want_R, want_sum = su.case_reference(Q, n, bits, True, C)
        qs, qm, _, _ = N.soft_query_planes(ops[0])
        rs, rn = N.pack_codes(ops[1])
        high = torch.tensor(-(1 << (bits % 32)), dtype=torch.int32, device=DEV)
        rs, rn, qm = rs.clone(), rn.clone(), qm.clone()
        rs[:, -1] |= high
        rn[:, -1] |= high
        qm[:, :, -1] |= high
        for k in (None, 50):
            ap, relevant, rank_sum = N.soft_ap((qs, qm), (rs, rn), bits, N.pack_labels(ops[2]), N.pack_labels(ops[3]), k)
            assert torch.equal(relevant.cpu(), torch.from_numpy(want_R).int()) and torch.equal(rank_sum.cpu(), torch.from_numpy(want_sum))
            _near(f"garbage bits={bits} k={k}", ap, want_ap[k])


@pytest.mark.parametrize("zeros", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1024, 1025, 2049, 4200])
def test_edges_of_the_item_walk(n, zeros):
    """One item, around a wave, one past a 256-item set of slabs, one chunk exactly, several chunks and a ragged last one; codes
    with and without zero entries."""
    _check_case(5, n, 64, zeros, 24)


@pytest.mark.parametrize("Q", [1, 2, 63, 64, 65, 130])
def test_query_counts_and_the_block_path(Q):
    """Up to SOFT_Q_MAX queries one call; 65 and 130: blocks, one mean over all of them; 32 bit: four queries share a workgroup, so
    the ragged last group of every count is walked too."""
    _check_case(Q, 1025, 32, True, 24)


@pytest.mark.parametrize("C", [1, 24, 33, 80])
def test_label_widths(C):
    """1..3 label words per item."""
    _check_case(9, 1025, 64, True, C)


def test_heavy_ties():
    """16 bit: eight queries share a workgroup.  Weights 15 and {0, +-1} through the quantiser; then weights in {0, +-1} alone, given
    as planes: at most 33 distinct distances among 2049 items, so the order is mostly the index order."""
    import cmh_native as N
    _check_case(9, 2049, 16, True, 24, "coarse")
    u, rB, qL, rL = su.case(9, 2049, 16, True, 24, "coarse")
    w = np.rint(u * 15).astype(np.int64)
    w[:, 0] = np.sign(w[:, 0])
    assert (np.abs(w) <= 1).all() and w[1:].any()
    ks = su.k_values(qL, rL)
    want_ap, want_R, want_sum = su.restated_w(w, rB, qL, rL, ks)
    sign, mag = softutil.planes(w)
    rp, ql, rl = N.pack_codes(_t(rB)), N.pack_labels(_t(qL)), N.pack_labels(_t(rL))
    for k in ks:
        ap, relevant, rank_sum = N.soft_ap((_t(sign), _t(mag)), rp, 16, ql, rl, k)
        assert torch.equal(relevant.cpu(), torch.from_numpy(want_R).int()) and torch.equal(rank_sum.cpu(), torch.from_numpy(want_sum))
        _near(f"weights in {{0, +-1}} k={k}", ap, want_ap[k])


def test_all_zero_query_ranks_by_index():
    """Every item at distance 0: rank = index + 1, so rank_sum and AP follow from the labels alone."""
    from utils.retrieval import soft_mean_average_precision
    u, rB, qL, rL = su.case(5, 1025, 64, True, 24)
    rel = mu.relevance(qL, rL)[1]                                        # (query 1's labels on an all-zero query)
    pos = np.nonzero(rel)[0] + 1
    _, ap, relevant, rank_sum = soft_mean_average_precision(_t(np.zeros((1, 64), np.float32)), _t(rB), _t(qL[1:2]), _t(rL), return_ap=True)
    assert int(relevant[0]) == len(pos) and int(rank_sum[0]) == int(pos.sum())
    assert abs(float(ap[0]) - (np.arange(1, len(pos) + 1) / pos).mean()) <= TOL_REF


@pytest.mark.parametrize("zeros", [False, True])
def test_saturated_queries_are_the_binary_map(zeros):
    """u = c * (a code without zeros): wdist = 15 h, so R and the ranks are those of mean_average_precision on that code.  relevant
    is exact; both APs lie within TOL_REF of the float64 restatement (each side's bound).  Bit-equality is printed, not asserted: the
    float64 terms meet in another order."""
    from utils.retrieval import mean_average_precision, soft_mean_average_precision
    Q, n, bits, C = 65, 2049, 64, 24
    qB = mu.case(Q, n, bits, False, C)[0]
    _, rB, qL, rL = mu.case(Q, n, bits, zeros, C)
    u = (qB * np.float32(0.37)).astype(np.float32)
    ks = (None, 1, 50)
    ref = mu.restated_ap(qB, rB, qL, rL, ks)
    ops = [_t(x) for x in (rB, qL, rL)]
    for k in ks:
        mp, ap, relevant, _ = soft_mean_average_precision(_t(u), *ops, k=k, return_ap=True)
        b_mp, b_ap = mean_average_precision(_t(qB), *ops, k=k, return_ap=True)
        assert torch.equal(relevant.cpu(), torch.from_numpy(mu.relevance(qL, rL).sum(1)).int())
        _near(f"saturated soft k={k}", ap, ref[k][0], mp)
        _near(f"saturated binary k={k}", b_ap, ref[k][0], b_mp)
        print(f"saturated k={k}: {int((ap == b_ap).sum())} of {Q} APs bit-equal, mAP bit-equal: {bool(mp == b_mp)}")


@pytest.mark.parametrize("k", [1, 50, 2049])
def test_cross_route_through_soft_topk_with_labels(k):
    """AP@k recomputed on the host from soft_topk's rel and cmh_soft_ap's relevant.  AP@k takes the first min(k, R) relevant items
    WHEREVER they rank (utils/calc_utils.py: total = min(k, R)), so the page that holds them is the whole database: 2049 items, three
    chunks, every k <= SOFT_K_MAX.  rel against the restatement's flags; without labels the returns are today's three."""
    from utils.retrieval import soft_mean_average_precision, soft_topk, soft_topn_precision
    Q, n, bits, C = 9, 2049, 64, 24
    u, rB, qL, rL = su.case(Q, n, bits, True, C)
    ops = [_t(x) for x in (u, rB, qL, rL)]
    plain = soft_topk(ops[0], ops[1], n)
    got = soft_topk(ops[0], ops[1], n, query_L=ops[2], retrieval_L=ops[3])
    assert len(plain) == 3 and len(got) == 4 and all(torch.equal(a, b) for a, b in zip(plain, got))
    rel = got[-1]
    assert rel.dtype == torch.uint8 and rel.shape == (Q, n)
    want_idx = softutil.topk(u, rB, n)[0]
    assert np.array_equal(rel.cpu().numpy().astype(bool), np.take_along_axis(mu.relevance(qL, rL), want_idx.astype(np.int64), 1))
    _, ap, relevant, rank_sum = soft_mean_average_precision(*ops, k=k, return_ap=True)
    hits = rel.cpu().numpy().astype(bool)
    assert np.array_equal(hits.sum(1), relevant.cpu().numpy())
    for q in range(Q):
        total = min(k, int(relevant[q]))
        pos = (np.nonzero(hits[q])[0] + 1).astype(np.float64)
        assert int(rank_sum[q]) == int(pos.sum())
        want = (np.arange(1, total + 1) / pos[:total]).sum() / total if total else 0.0
        assert abs(float(ap[q]) - want) <= TOL_REF, (q, k)
    if k == 50:
        precision, recall, rel50 = soft_topn_precision(*ops, topn=(1, 10, 50))
        assert torch.equal(rel50, rel[:, :50])
        keep = relevant.cpu().numpy() > 0
        cum = hits[keep].cumsum(1)[:, [0, 9, 49]].astype(np.float64)
        assert np.allclose(precision.numpy(), (cum / np.array([1, 10, 50])).mean(0), rtol=0, atol=1e-15)
        assert np.allclose(recall.numpy(), (cum / relevant.cpu().numpy()[keep][:, None]).mean(0), rtol=0, atol=1e-15)


def test_masked_soft_topk_with_labels_pads_rel_with_zero():
    from utils.retrieval import ItemMask, soft_topk
    u, rB, qL, rL = su.case(5, 257, 64, True, 24)
    ops = [_t(x) for x in (u, rB, qL, rL)]
    mask = ItemMask.from_ids(257, torch.arange(0, 20), keep=True, device=DEV)
    idx, dist, wdist, found, rel = soft_topk(ops[0], ops[1], 50, mask=mask, query_L=ops[2], retrieval_L=ops[3])
    assert (found == 20).all() and (idx[:, 20:] == -1).all() and (rel[:, 20:] == 0).all()
    want = mu.relevance(qL, rL)
    assert np.array_equal(rel[:, :20].cpu().numpy().astype(bool), np.take_along_axis(want, idx[:, :20].cpu().numpy().astype(np.int64), 1))


def test_two_calls_two_streams_and_blocks_give_equal_bytes():
    import cmh_native as N
    Q, n, bits, C = 64, 4200, 64, 24
    u, rB, qL, rL = su.case(Q, n, bits, True, C)
    q = N.soft_query_planes(_t(u))
    rp, ql, rl = N.pack_codes(_t(rB)), N.pack_labels(_t(qL)), N.pack_labels(_t(rL))
    for k in (None, 50):
        first = N.soft_ap(q, rp, bits, ql, rl, k)
        again = N.soft_ap(q, rp, bits, ql, rl, k)
        torch.cuda.synchronize()
        outs = []
        for _ in range(2):
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                outs.append(N.soft_ap(q, rp, bits, ql, rl, k))
        torch.cuda.synchronize()
        singles = [N.soft_ap((q[0][i:i + 1], q[1][i:i + 1]), rp, bits, ql[i:i + 1], rl, k) for i in range(0, Q, 7)]
        for other in [again] + outs:
            assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(first, other))
        for j, i in enumerate(range(0, Q, 7)):
            assert all(torch.equal(a[i:i + 1].view(torch.uint8), b.view(torch.uint8)) for a, b in zip(first, singles[j]))


def test_code_index_map_soft_after_add():
    from utils.retrieval import CodeIndex, soft_mean_average_precision
    import cmh_native as N
    Q, n, bits, C = 65, 2049, 64, 24
    u, rB, qL, rL = su.case(Q, n, bits, True, C)
    ops = [_t(x) for x in (u, rB, qL, rL)]
    index = CodeIndex(ops[1][:700], ops[3][:700])
    index.add(ops[1][700:701], ops[3][700:701]).add(ops[1][701:], ops[3][701:])
    for k in (None, 50):
        want = soft_mean_average_precision(*ops, k=k, return_ap=True)
        got = index.map_soft(ops[0], ops[2], k=k, return_ap=True)
        assert all(torch.equal(a, b) for a, b in zip(want, got))
        assert torch.equal(index.map_soft(ops[0], ops[2], k=k), want[0])
    plain = index.search_soft(ops[0], 50)
    got = index.search_soft(ops[0], 50, query_labels=ops[2])
    assert len(got) == 4 and all(torch.equal(a, b) for a, b in zip(plain, got))
    hits = np.take_along_axis(mu.relevance(qL, rL), got[0].cpu().numpy().astype(np.int64), 1)
    assert np.array_equal(got[3].cpu().numpy().astype(bool), hits)
    with pytest.raises(N.NativeError, match="CodeIndex.map_soft: needs query labels of 24 classes"):
        index.map_soft(ops[0], None)
    with pytest.raises(N.NativeError, match="CodeIndex.map_soft: 32-entry soft queries"):
        index.map_soft(ops[0][:, :32], ops[2])
    with pytest.raises(N.NativeError, match="CodeIndex.map_soft: the index holds no labels"):
        CodeIndex(ops[1]).map_soft(ops[0], ops[2])
    with pytest.raises(N.NativeError, match="CodeIndex.search_soft: query labels given, but the index has none"):
        CodeIndex(ops[1]).search_soft(ops[0], 5, query_labels=ops[2])


def test_refusals_by_message():
    import cmh_native as N
    from utils.retrieval import soft_mean_average_precision
    u, rB, qL, rL = su.case(5, 257, 64, True, 24)
    ops = [_t(x) for x in (u, rB, qL, rL)]
    q = N.soft_query_planes(ops[0])
    rp, ql, rl = N.pack_codes(ops[1]), N.pack_labels(ops[2]), N.pack_labels(ops[3])
    for k in (0, 258, -3):
        with pytest.raises(N.NativeError, match=f"soft_ap: k={k} outside"):
            N.soft_ap(q, rp, 64, ql, rl, k)
        with pytest.raises(N.NativeError, match=f"soft_mean_average_precision: k={k} outside"):
            soft_mean_average_precision(*ops, k=k)
    with pytest.raises(N.NativeError, match="soft_ap: operand of shape"):
        N.soft_ap(q, rp, 64, ql[:4], rl)
    with pytest.raises(N.NativeError, match="soft_ap: packed operands are contiguous int32"):
        N.soft_ap(q, rp, 64, ql.long(), rl.long())
    bad = ops[0].clone()
    bad[2, 5] = float("nan")
    with pytest.raises(N.NativeError, match="a soft query must be finite"):
        soft_mean_average_precision(bad, *ops[1:])
    # the C ABI itself: 65 queries in one call, and a workspace one byte short
    lib = N.lib()
    out = torch.zeros(65 * 2, dtype=torch.int64, device=DEV)
    ws = N.workspace(8 << 20, DEV, "test_soft_ap")
    args = lambda Q, nbytes: (N.ptr(q[0]), N.ptr(q[1]), N.ptr(rp[0]), N.ptr(rp[1]), N.ptr(ql), N.ptr(rl), 1, Q, 257, 64, 0,
                              N.ptr(out), N.ptr(out), N.ptr(out), N.ptr(ws), nbytes, None)
    assert lib.cmh_soft_ap(*args(65, 8 << 20)) == -1 and b"soft_ap: Q=65" in lib.cmh_last_error()
    need = lib.cmh_soft_ap_workspace_bytes(5, 257, 64, 1)
    assert 0 < need <= (8 << 20)
    assert lib.cmh_soft_ap(*args(5, need - 1)) == -2 and b"soft_ap: workspace" in lib.cmh_last_error()


def test_trainer_eval_soft(tmp_path, monkeypatch):
    """A short DSPH run on the synthetic set (the configuration of the other end-to-end tests), then test() from its checkpoint
    without and with --eval-soft: the log holds the four lines, the .mat arrays equal the library calls on the stored soft_q_* and
    codes, the plain keys are those of the run without the flag; a MITH run refuses the flag by name."""
    import argparse
    import sys
    import scipy.io as scio
    import main
    import recipe
    import dataset.synthetic as ds
    from utils import retrieval as R
    ck = tmp_path / "clip.pt"
    torch.save({k: torch.from_numpy(v) for k, v in recipe.clip_state_dict(recipe.CLIP_TINY, 7).items()}, ck)
    monkeypatch.setattr(ds, "SOT", 510); monkeypatch.setattr(ds, "EOT", 511)
    common = ["main.py", "-clip-path", str(ck), "--batch-size", "16", "--num-workers", "0", "--resolution", "64",
              "--max-words", "16", "--query-num", "24", "--train-num", "32", "--synthetic-size", "120", "--gemm-dtype", "f32"]
    monkeypatch.setattr(sys, "argv", common + ["--save-dir", str(tmp_path / "run"), "--epochs", "1"])
    main.trainers["DSPH"](argparse.Namespace(method="DSPH", dataset="synthetic", output_dim=16, is_train=True), 0)
    model = tmp_path / "run" / "DSPH" / "synthetic" / "16" / "model-0.pth"
    assert model.exists()
    runs = {}
    for tag, extra in (("plain", []), ("soft", ["--eval-soft", "true"])):
        monkeypatch.setattr(sys, "argv", common + ["--save-dir", str(tmp_path / tag), "--pretrained", str(model)] + extra)
        main.trainers["DSPH"](argparse.Namespace(method="DSPH", dataset="synthetic", output_dim=16, is_train=False), 0)
        path = tmp_path / tag / "DSPH" / "synthetic" / "16" / "PR_cruve" / "16-ours-synthetic-i2t.mat"
        log = open(tmp_path / tag / "DSPH" / "synthetic" / "16" / "test.log").read()
        runs[tag] = ({k: v for k, v in scio.loadmat(path).items() if not k.startswith("__")}, log)
    plain, rec = runs["plain"][0], runs["soft"][0]
    assert set(plain) == {"q_img", "q_txt", "r_img", "r_txt", "q_l", "r_l"}
    for k in plain:
        np.testing.assert_array_equal(plain[k], rec[k])
    dirs = {"i2t": ("img", "txt"), "t2i": ("txt", "img"), "i2i": ("img", "img"), "t2t": ("txt", "txt")}
    names = ("ap", "map", "auc", "rank_sum", "relevant", "topn_precision")
    assert set(rec) - set(plain) == {"soft_q_img", "soft_q_txt", "soft_topn"} | {f"soft_{n}_{d}" for n in names for d in dirs}
    Q, n = plain["q_img"].shape[0], plain["r_img"].shape[0]
    topn = [int(t) for t in rec["soft_topn"].ravel()]
    assert topn == [t for t in R.DEFAULT_TOPN if t <= n] and rec["soft_q_img"].dtype == np.float32
    qL, rL = _t(plain["q_l"].astype(np.float32)), _t(plain["r_l"].astype(np.float32))
    for d, (qs, rs) in dirs.items():
        u, q, r = _t(rec[f"soft_q_{qs}"]), _t(plain[f"q_{qs}"].astype(np.float32)), _t(plain[f"r_{rs}"].astype(np.float32))
        assert torch.equal(torch.sign(u), q)                              # the stored codes are the sign of the stored soft outputs
        mp, ap, relevant, rank_sum = R.soft_mean_average_precision(u, r, qL, rL, return_ap=True)
        np.testing.assert_array_equal(rec[f"soft_ap_{d}"].ravel(), ap.cpu().numpy())
        np.testing.assert_array_equal(rec[f"soft_relevant_{d}"].ravel(), relevant.cpu().numpy())
        np.testing.assert_array_equal(rec[f"soft_rank_sum_{d}"].ravel(), rank_sum.cpu().numpy())
        assert rec[f"soft_rank_sum_{d}"].dtype == np.int64 and float(rec[f"soft_map_{d}"].ravel()[0]) == float(mp)
        np.testing.assert_array_equal(rec[f"soft_auc_{d}"].ravel(), R.auc_from_rank_sum(rank_sum, relevant, n).numpy())
        tp = R.soft_topn_precision(u, r, qL, rL, topn)[0]
        np.testing.assert_array_equal(rec[f"soft_topn_precision_{d}"].ravel(), tp.numpy())
        b_mp = R.mean_average_precision(q, r, qL, rL)
        b_tp = R.topn_precision(q, r, qL, rL, topn)[0]
        at = topn.index(100) if 100 in topn else len(topn) - 1
        line = (f">>>>>> soft({d}): mAP: {float(mp):.6f} (binary, ties by index: {float(b_mp):.6f}), "
                f"AUC: {float(torch.nanmean(R.auc_from_rank_sum(rank_sum, relevant, n))):.6f}, "
                f"P@{topn[at]}: {float(tp[at]):.6f} (binary: {float(b_tp[at]):.6f})")
        assert line in runs["soft"][1], line
    assert "soft(" not in runs["plain"][1]
    monkeypatch.setattr(sys, "argv", common + ["--save-dir", str(tmp_path / "mith"), "--pretrained", str(model), "--eval-soft", "true"])
    with pytest.raises(ValueError, match="--eval-soft: method MITH has no soft rule"):
        main.trainers["MITH"](argparse.Namespace(method="MITH", dataset="synthetic", output_dim=16, is_train=False), 0)
