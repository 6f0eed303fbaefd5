"""mAP by counting on the GPU (cmh_hamming_ap_partial / cmh_ap_finish, utils.retrieval.mean_average_precision, CodeIndex.map,
calc_map_k_matrix(tie_order="stable") past the ranking's limit, retrieve.py --map, --map-tie-order stable) against the float64
restatement of tests/mapcountutil.py, against the stable ranking kernel, over shards, and twice for equal bits.

Bounds.  Against the restatement, 2.4e-7 on every AP and on the mAP: a term relrank / rank is one f32 quotient (<= 6e-8 relative,
terms <= 1), the float64 sum of the terms is exact at these sizes, the quotient by `total` is rounded to f32 once: two f32 ulps at 1.
Against the ranking kernel 2e-6, the tolerance of tests/test_gpu_map.py.  Sharded against unsharded one f32 ulp at 1 (1.2e-7): the
float64 sums are the same terms in another grouping."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mapcountutil as mu
from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_REF, TOL_RANKING, TOL_SHARD = 2.4e-7, 2e-6, 1.2e-7


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check(tag, got_map, got_ap, want_ap, want_map, tol=TOL_REF):
    d_ap = float(np.abs(got_ap.cpu().numpy().astype(np.float64) - want_ap).max())
    d_map = abs(float(got_map) - want_map)
    print(f"{tag}: max|ap - ref| = {d_ap:.3e}, |mAP - ref| = {d_map:.3e}")
    assert d_ap <= tol and d_map <= tol, (tag, d_ap, d_map)


# (Q, N, bits, zeros, classes): Q 1 / 63 / 64 / 65 / 130 (ragged last tile, lanes that repeat the last query); N 1 / 3 / 63 / 65 (fewer
# items than a Group, ragged tails) / 1000 / 70 000 (many chunks); bits 16 / 64 / 96 / 128 (1..4 words in registers) and 192 (columns
# in the workspace); classes 4 (one label word), 80 (three), 100 (staged).
SHAPES = [(1, 1, 16, False, 4), (1, 1000, 64, True, 4), (63, 3, 16, True, 4), (64, 63, 64, False, 4), (65, 65, 96, True, 80),
          (130, 1000, 128, False, 4), (130, 1000, 64, True, 100), (63, 1000, 16, True, 80), (64, 1000, 96, False, 100),
          (65, 1000, 192, True, 4), (3, 1000, 192, False, 100), (130, 70000, 64, False, 4), (5, 70000, 128, True, 80),
          (2, 70000, 16, False, 4), (2, 70000, 192, True, 4)]


@pytest.mark.parametrize("Q,N,bits,zeros,C", SHAPES)
def test_ap_by_counting_matches_the_float64_restatement(Q, N, bits, zeros, C):
    from utils.retrieval import mean_average_precision
    qB, rB, qL, rL = mu.case(Q, N, bits, zeros, C)
    mu.check_label_mix(qL, rL)
    ref = mu.case_reference(Q, N, bits, zeros, C)
    ops = [_t(x) for x in (qB, rB, qL, rL)]
    for k, (want_ap, want_map) in ref.items():
        mp, ap = mean_average_precision(*ops, k=k, return_ap=True)
        assert mp.dtype == torch.float32 and mp.dim() == 0 and not mp.is_cuda and ap.dtype == torch.float32 and ap.shape == (Q,)
        _check(f"Q={Q} N={N} bits={bits} zeros={zeros} C={C} k={k}", mp, ap, want_ap, want_map)
        assert float(ap[-1]) == 0.0 or Q == 1                          # the query without labels
    if Q == 1:                                                         # one query cannot be both: the same case with no label at all
        none = np.zeros_like(qL)
        mp, ap = mean_average_precision(ops[0], ops[1], _t(none), ops[3], return_ap=True)
        assert float(mp) == 0.0 and float(ap[0]) == 0.0


def _special(kind):
    Q, N, bits, C = 65, 1000, 64, 4
    rng = np.random.default_rng(["identical", "all_relevant", "relevant_last"].index(kind) + 77)
    qL, rL = mu.labels(rng, Q, N, C)
    qB, rB = mu.codes(rng, Q, bits, True), mu.codes(rng, N, bits, True)
    if kind == "identical":                                            # one bin: AP depends on the index order alone
        rB[:] = rB[0].copy()
    elif kind == "all_relevant":
        rL[:] = 1.0
        qL[:-1, 0] = 1.0
    else:                                                              # the relevant items are exactly those at the largest h = 2K
        c = mu.codes(rng, 1, bits, False)
        qB[:] = c
        rL[:] = 0.0
        rL[::3, 0] = 1.0
        rL[1::3, 1] = 1.0
        qL[:] = 0.0
        qL[:40, 0] = 1.0
        qL[40:50, 2] = 1.0
        rB[:, 0] = c[0, 0]                                             # an entry that agrees (or is 0): h < 2K
        rB[::3] = -c
        assert (mu.half_units(qB, rB)[0][::3] == 2 * bits).all() and (mu.half_units(qB, rB)[0] == 2 * bits).sum() == len(rB[::3])
    return qB, rB, qL, rL


@pytest.mark.parametrize("kind", ["identical", "all_relevant", "relevant_last"])
def test_special_databases(kind):
    from utils.retrieval import mean_average_precision
    qB, rB, qL, rL = _special(kind)
    mu.check_label_mix(qL, rL)
    ks = mu.k_values(qL, rL)
    ref = mu.restated_ap(qB, rB, qL, rL, ks)
    ops = [_t(x) for x in (qB, rB, qL, rL)]
    for k in ks:
        mp, ap = mean_average_precision(*ops, k=k, return_ap=True)
        _check(f"{kind} k={k}", mp, ap, *ref[k])
    if kind == "all_relevant":                                         # every rank is its own relrank: AP = 1 exactly
        assert (mean_average_precision(*ops, return_ap=True)[1][:-1] == 1.0).all()


@pytest.mark.parametrize("Q,N,bits,zeros,C", [(64, 63, 64, False, 4), (65, 65, 96, True, 80), (130, 1000, 64, True, 100),
                                              (65, 1000, 192, True, 4), (130, 70000, 64, False, 4)])
def test_ap_by_counting_matches_the_stable_ranking_kernel(Q, N, bits, zeros, C):
    import cmh_native as Nn
    from utils.retrieval import mean_average_precision
    qB, rB, qL, rL = mu.case(Q, N, bits, zeros, C)
    ops = [_t(x) for x in (qB, rB, qL, rL)]
    qp, rp, ql, rl = Nn.pack_codes(ops[0]), Nn.pack_codes(ops[1]), Nn.pack_labels(ops[2]), Nn.pack_labels(ops[3])
    for k in mu.k_values(qL, rL)[:5]:                                  # (the ranking takes no k above N)
        want_map, want_ap, _ = Nn.hamming_map(qp, ql, rp, rl, bits, C, topk=k, tie_order=Nn.TIE_STABLE)
        mp, ap = mean_average_precision(*ops, k=k, return_ap=True)
        _check(f"vs ranking Q={Q} N={N} bits={bits} k={k}", mp, ap, want_ap.cpu().numpy().astype(np.float64), float(want_map), TOL_RANKING)


SHARDED = (65, 2300, 64, True, 4)


@pytest.mark.parametrize("shard_items", [7, 100, 1000])
def test_shards_add_up_to_the_unsharded_call(shard_items):
    from utils.retrieval import mean_average_precision
    qB, rB, qL, rL = mu.case(*SHARDED)
    mu.check_label_mix(qL, rL)
    ops = [_t(x) for x in (qB, rB, qL, rL)]
    ref = mu.case_reference(*SHARDED)
    for k in mu.k_values(qL, rL):
        one_map, one_ap = mean_average_precision(*ops, k=k, return_ap=True)
        mp, ap = mean_average_precision(*ops, k=k, shard_items=shard_items, return_ap=True)
        d = float((ap.double() - one_ap.double()).abs().max())
        print(f"shard_items={shard_items} k={k}: max|ap - unsharded| = {d:.3e}, |mAP - unsharded| = {abs(float(mp) - float(one_map)):.3e}")
        assert d <= TOL_SHARD and abs(float(mp) - float(one_map)) <= TOL_SHARD
        _check(f"shard_items={shard_items} k={k}", mp, ap, *ref[k])


@pytest.fixture(scope="module")
def big():
    """A database one native call cannot hold: 524 288 + 37 items of 16 bits, 3 queries."""
    Q, N, bits, C = 3, 524288 + 37, 16, 4
    qB, rB, qL, rL = mu.case(Q, N, bits, True, C)
    return (qB, rB, qL, rL), mu.restated_ap(qB, rB, qL, rL, (None, 50)), [_t(x) for x in (qB, rB, qL, rL)]


def test_a_database_one_call_cannot_hold(big):
    import cmh_native as Nn
    from utils.calc_utils import calc_map_k_matrix
    from utils.retrieval import mean_average_precision
    (qB, rB, qL, rL), ref, ops = big
    mu.check_label_mix(qL, rL)
    for k in (None, 50):
        mp, ap = mean_average_precision(*ops, k=k, return_ap=True)
        _check(f"N={rB.shape[0]} k={k}", mp, ap, *ref[k])
        # calc_map_k_matrix: "stable" goes to the counting path above the ranking's limit, "reference" does not exist there
        mp2, ap2 = calc_map_k_matrix(*ops, k=k, return_ap=True, tie_order="stable")
        assert torch.equal(mp2, mp) and torch.equal(ap2, ap)
        assert torch.equal(calc_map_k_matrix(*ops, k=k, tie_order="stable"), mp)
    with pytest.raises(Nn.NativeError, match="stable"):
        calc_map_k_matrix(*ops)
    with pytest.raises(Nn.NativeError, match="stable"):
        calc_map_k_matrix(*ops, tie_order="reference")


def test_two_calls_with_explicit_total_and_prior_counts():
    import cmh_native as Nn
    Q, N, bits, zeros, C = SHARDED
    qB, rB, qL, rL = mu.case(*SHARDED)
    ref = mu.case_reference(*SHARDED)
    qp, rp, ql, rl = Nn.pack_codes(_t(qB)), Nn.pack_codes(_t(rB)), Nn.pack_labels(_t(qL)), Nn.pack_labels(_t(rL))
    cut = 1237
    a, b = tuple(x[:cut] for x in rp), tuple(x[cut:] for x in rp)
    total = Nn.hamming_hist(qp, rp, bits, ql, rl)
    first = Nn.hamming_hist(qp, a, bits, ql, rl[:cut])
    for k in (None, 5):
        sum_a, own_a = Nn.hamming_ap_partial(qp, a, bits, ql, rl[:cut], topk=k, total_counts=total, want_counts=True)
        sum_b, own_b = Nn.hamming_ap_partial(qp, b, bits, ql, rl[cut:], topk=k, total_counts=total, prior_counts=first, want_counts=True)
        assert sum_a.dtype == torch.float64 and torch.equal(own_a, first) and torch.equal(own_a + own_b, total)
        mp, ap = Nn.ap_finish(sum_a + sum_b, total, bits, topk=k)
        _check(f"two calls k={k}", mp, ap, *ref[k])
        whole, own = Nn.hamming_ap_partial(qp, rp, bits, ql, rl, topk=k, want_counts=True)
        assert torch.equal(own, total)
        assert float((sum_a + sum_b - whole).abs().max()) <= 1e-9 * max(1.0, float(whole.abs().max()))
    # without the histogram of the whole database a shard ranks against itself: another number (the operand is not ignored)
    alone = Nn.hamming_ap_partial(qp, b, bits, ql, rl[cut:])
    assert not torch.equal(alone, sum_b)


@pytest.mark.parametrize("Q,N,bits,zeros,C", [(130, 1000, 128, False, 4), (65, 1000, 192, True, 4), (130, 70000, 64, False, 4)])
def test_two_calls_give_equal_bits(Q, N, bits, zeros, C):
    from utils.retrieval import mean_average_precision
    ops = [_t(x) for x in mu.case(Q, N, bits, zeros, C)]
    mp, ap = mean_average_precision(*ops, return_ap=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        mp2, ap2 = mean_average_precision(*ops, return_ap=True)
        mp3, ap3 = mean_average_precision(*ops, shard_items=300, return_ap=True)
    side.synchronize()
    mp4, ap4 = mean_average_precision(*ops, shard_items=300, return_ap=True)
    assert torch.equal(mp, mp2) and torch.equal(ap, ap2) and torch.equal(mp3, mp4) and torch.equal(ap3, ap4)


def test_code_index_map_and_the_command_line(tmp_path):
    import scipy.io as scio
    import cmh_native as Nn
    from utils.retrieval import CodeIndex, mean_average_precision
    qB, rB, qL, rL = mu.case(*SHARDED)
    ops = [_t(x) for x in (qB, rB, qL, rL)]
    index = CodeIndex(ops[1][:900], ops[3][:900], shard_items=1000)
    index.add(ops[1][900:], ops[3][900:])
    index.save(str(tmp_path / "db.npz"))
    index = CodeIndex.load(str(tmp_path / "db.npz"), shard_items=1000)
    for k in (None, 50):
        want = mean_average_precision(*ops, k=k, shard_items=1000, return_ap=True)
        got = index.map(ops[0], ops[2], k=k, return_ap=True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert torch.equal(index.map(ops[0], ops[2], k=k), want[0])
    with pytest.raises(Nn.NativeError, match="labels"):
        CodeIndex(ops[1]).map(ops[0], ops[2])
    # retrieve.py --map in a fresh process: the same number, against the file's database side and against the saved index
    path = tmp_path / "codes.mat"
    scio.savemat(str(path), {"q_img": qB, "q_txt": qB, "r_img": rB, "r_txt": rB, "q_l": qL, "r_l": rL})
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for extra, k in (([], None), (["--k", "50"], 50), (["--index", str(tmp_path / "db.npz")], None)):
        out = subprocess.run([sys.executable, os.path.join(PKG, "retrieve.py"), "--codes", str(path), "--direction", "i2t", "--map"] + extra,
                             capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
        assert out.returncode == 0, out.stderr[-2000:]
        lines = out.stdout.strip().splitlines()
        assert len(lines) == 1
        assert float(lines[0]) == float(f"{float(mean_average_precision(*ops, k=k)):.8f}")


def test_trainer_logs_the_stable_map(tmp_path, monkeypatch):
    """A DSPH trainer on the synthetic set with --map-tie-order stable: valid() logs four mAPs, those of
    calc_map_k_matrix(tie_order="stable") on the codes it saved; the default logs the reference order's."""
    import argparse
    import re
    import recipe
    import scipy.io as scio
    import main
    import dataset.synthetic as ds
    from utils.calc_utils import calc_map_k_matrix
    ck = tmp_path / "clip.pt"
    torch.save({k: torch.from_numpy(v) for k, v in recipe.clip_state_dict(recipe.CLIP_TINY, 7).items()}, ck)
    monkeypatch.setattr(ds, "SOT", 510); monkeypatch.setattr(ds, "EOT", 511)
    monkeypatch.setattr(sys, "argv", ["main.py", "-clip-path", str(ck), "--save-dir", str(tmp_path / "run"), "--batch-size", "16",
                                      "--num-workers", "0", "--resolution", "64", "--max-words", "16", "--query-num", "24",
                                      "--train-num", "32", "--synthetic-size", "120", "--gemm-dtype", "f32", "--epochs", "0",
                                      "--map-tie-order", "stable"])
    torch.manual_seed(1)
    tr = main.trainers["DSPH"](argparse.Namespace(method="DSPH", dataset="synthetic", output_dim=16, is_train=True), 0)
    assert tr.args.map_tie_order == "stable"
    got = tr.valid(0)
    run = tmp_path / "run" / "DSPH" / "synthetic" / "16"
    m = scio.loadmat(str(run / "PR_cruve" / "16-ours-synthetic-i2t.mat"))
    c = {k: torch.from_numpy(m[k]).float() for k in ("q_img", "q_txt", "r_img", "r_txt", "q_l", "r_l")}
    want = [calc_map_k_matrix(c[a], c[b], c["q_l"], c["r_l"], tie_order="stable")
            for a, b in (("q_img", "r_txt"), ("q_txt", "r_img"), ("q_img", "r_img"), ("q_txt", "r_txt"))]
    assert len(got) == 4
    for g, w in zip(got, want):
        assert abs(float(g) - float(w)) <= 2e-6, (float(g), float(w))
    line = [ln for ln in open(run / "train.log").read().splitlines() if "MAP(i->t)" in ln][-1]
    logged = [float(v) for v in re.findall(r"MAP\((?:i->t|t->i|t->t|i->i)\): ([0-9.e-]+)", line)[:4]]
    assert len(logged) == 4
    for v, w in zip(logged, (want[0], want[1], want[3], want[2])):      # (the line's order: i->t, t->i, t->t, i->i)
        assert abs(v - float(w)) <= 2e-6, (v, float(w))
