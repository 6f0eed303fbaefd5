"""The bucket table on the GPU (csrc/retrieval_buckets.hip: cmh_code_sort, cmh_code_bucket_count / _fill, cmh_bucket_probe_count /
_fill; utils/retrieval.py::BucketTable, CodeIndex.buckets / lookup / bucket_stats; main.py --eval-buckets) against the NumPy
restatement of tests/bucketutil.py.  Everything is an integer, an index or a whole-bit distance: every comparison is exact.

The 16-bit lookup case: a 16-bit code has 137 keys within radius 2, so a ball cannot hold more buckets than that; the case's
database is a centre code with at most two bits flipped, and the centre's ball hits them all."""
import sys

import numpy as np
import pytest
import torch

import bucketutil as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _sign_plane(N, bits, draw, seed):
    """The case's sign plane as the sort gets it: pack_codes' plane, the plane-level edit of topbit / lastbit, and random bits ORed
    in behind `bits` (they must not matter) -> int32 [N, W] on the GPU."""
    import cmh_native as Nv
    sign = Nv.pack_codes(_t(U.draw_codes(N, bits, draw, seed)))[0].clone()
    edit = U.edit_bit(N, bits, draw, seed)
    if edit is not None:
        word, bit, flips = edit
        flip = torch.tensor(np.array([1 << bit], dtype=np.uint32).view(np.int32), device=DEV)
        sign[:, word] = (sign[:, word] & ~flip) | torch.where(_t(flips), flip, torch.zeros_like(flip))      # set / cleared, not toggled
    if bits % 32:
        rng = np.random.default_rng(seed + 2)
        garbage = rng.integers(0, 1 << 32, size=N, dtype=np.uint64).astype(np.uint32) & ~U.word_masks(bits)[-1]
        sign[:, -1] |= _t(garbage.view(np.int32))
    return sign.contiguous()


@pytest.mark.parametrize("N,bits,draw", U.SORT_CASES)
def test_sort_and_buckets_equal_the_restatement(N, bits, draw):
    import cmh_native as Nv
    assert Nv.SORT_TILE == U.SORT_TILE
    sign = _sign_plane(N, bits, draw, seed=1000 + N + bits)
    words = U.keys(sign.cpu().numpy(), bits)
    want_order = U.ref_order(words)
    want_starts, want_codes = U.ref_buckets(words)
    if draw in ("topbit", "lastbit") and N >= 2:
        clear = int((~U.edit_bit(N, bits, draw, 1000 + N + bits)[2]).sum())
        assert want_starts.size == 3 and want_order[clear] == 0   # two keys; item 0 leads the larger one's bucket (unsigned order)
    order = Nv.code_sort(sign, bits)
    starts, codes = Nv.code_buckets(sign, order, bits)
    assert order.dtype == torch.int32 and starts.dtype == torch.int32 and codes.dtype == torch.int32
    np.testing.assert_array_equal(order.cpu().numpy(), want_order)
    assert codes.shape[0] == want_codes.shape[0]                   # n_buckets
    np.testing.assert_array_equal(starts.cpu().numpy(), want_starts)
    np.testing.assert_array_equal(codes.cpu().numpy().view(np.uint32), want_codes)
    again = Nv.code_sort(sign, bits)
    starts2, codes2 = Nv.code_buckets(sign, again, bits)
    assert torch.equal(order, again) and torch.equal(starts, starts2) and torch.equal(codes, codes2)


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and torch.equal(g, w)


@pytest.mark.parametrize("radius", [0, 1, 2])
@pytest.mark.parametrize("Q", [1, 65])
@pytest.mark.parametrize("name", sorted(U.LOOKUP_CASES))
def test_lookup_equals_range_search(name, Q, radius):
    from utils.retrieval import BucketTable, CodeIndex
    rB, rL, qB, qL = U.lookup_case(name, Q)
    index = CodeIndex(_t(rB), _t(rL))
    want = index.range_search(_t(qB), radius, _t(qL))
    got = index.lookup(_t(qB), radius, _t(qL))
    assert len(got) == 4
    _same(got, want)
    _same(index.lookup(_t(qB), radius), index.range_search(_t(qB), radius))
    ref = U.ref_lookup(qB, rB, radius, qL, rL)
    for g, r in zip(got, ref):
        np.testing.assert_array_equal(g.cpu().numpy(), r)
    balls = np.diff(ref[0])
    if Q > 1:
        assert (balls == 0).any() or name == "dense16"            # empty balls are among the cases (a 3-bit flip of a sparse code)
    if name == "dense16" and radius == 2:
        assert index.buckets().n_buckets == 137 and balls[0] == rB.shape[0]      # the centre's ball: every key, every item
    table = BucketTable.build(index.planes, index.bits)            # the module-level form, labels as multi-hot matrices
    _same(table.lookup(_t(qB), radius, _t(qL), _t(rL)), want)


def test_three_flipped_bits_of_distinct_codes_find_nothing():
    from utils.retrieval import CodeIndex
    rng = np.random.default_rng(5)
    rB = (rng.integers(0, 2, size=(3000, 64)) * 2 - 1).astype(np.float32)
    qB = rB[:70].copy()
    for i in range(70):
        qB[i, rng.choice(64, size=3, replace=False)] *= -1
    assert U.ref_lookup(qB, rB, 2)[0][-1] == 0                     # the restatement: nothing within 2 bits
    index = CodeIndex(_t(rB))
    off, idx, dist = index.lookup(_t(qB), 2)
    assert torch.equal(off, torch.zeros(71, dtype=torch.int64, device=DEV)) and idx.numel() == 0 and dist.numel() == 0
    assert idx.dtype == torch.int32 and dist.dtype == torch.float32
    _same((off, idx, dist), index.range_search(_t(qB), 2))
    assert torch.equal(index.lookup(_t(rB[:70]), 0)[1].long(), torch.arange(70, device=DEV))      # unflipped, each finds itself alone


def test_own_codes_at_radius_zero_are_the_duplicates():
    from utils.retrieval import CodeIndex
    rB, rL, _, _ = U.lookup_case("ties64", 1)
    index = CodeIndex(_t(rB), _t(rL))
    off, idx, dist, rel = index.lookup(_t(rB), 0, _t(rL))
    ball = off[1:] - off[:-1]
    item = torch.repeat_interleave(torch.arange(index.size, device=DEV), ball)
    keep = idx != item
    assert int((~keep).sum()) == index.size                        # every item finds itself, once
    out = torch.zeros_like(off)
    torch.cumsum(ball - 1, 0, out=out[1:])
    _same((out, idx[keep], dist[keep], rel[keep]), index.duplicates(0))


def test_bucket_stats_count_the_distinct_codes():
    from utils.retrieval import CodeIndex
    for name in sorted(U.LOOKUP_CASES):
        rB = U.lookup_case(name, 1)[0]
        st = CodeIndex(_t(rB)).bucket_stats()
        uniq, counts = torch.unique(_t(rB), dim=0, return_counts=True)
        assert st["distinct"] == uniq.shape[0] and st["n"] == rB.shape[0] and st["largest"] == int(counts.max())
        assert st["singletons"] == int((counts == 1).sum()) and st["collisions"] == int((counts * (counts - 1) // 2).sum())
        assert int((st["occupancy"][:, 0] * st["occupancy"][:, 1]).sum()) == rB.shape[0]
        assert st["used_share"] == uniq.shape[0] / min(rB.shape[0], 2 ** rB.shape[1])


def test_the_table_is_rebuilt_after_add():
    from utils.retrieval import CodeIndex
    rB = U.lookup_case("wide128", 1)[0]
    index = CodeIndex(_t(rB[:200]))
    first = index.buckets()
    assert index.buckets() is first                                # kept between calls
    new = rB[200:].copy()
    new[0] = -rB[0]                                                # a code the index has not seen
    before = index.lookup(_t(new[:1]), 0)
    assert before[1].numel() == 0
    index.add(_t(new))
    assert index.buckets() is not first and index.buckets().n == rB.shape[0]
    after = index.lookup(_t(new[:1]), 0)
    assert after[1].cpu().tolist() == [200]
    _same(index.lookup(_t(rB[:33]), 1), index.range_search(_t(rB[:33]), 1))


def test_refusals_name_the_limit_before_a_launch(monkeypatch):
    import cmh_native as Nv
    from utils.retrieval import BucketTable, CodeIndex
    rB = U.lookup_case("wide128", 1)[0]
    launched = []
    for name in ("code_sort", "bucket_probe_count", "bucket_probe_fill"):
        monkeypatch.setattr(Nv, name, lambda *a, _n=name, **k: launched.append(_n))
    zero = rB.copy()
    zero[3, 5] = 0
    with pytest.raises(Nv.NativeError, match=r"0 entry.*\{-1, \+1\}"):
        CodeIndex(_t(zero)).buckets()
    with pytest.raises(Nv.NativeError, match=r"0 entry.*\{-1, \+1\}"):
        CodeIndex(_t(zero)).lookup(_t(rB[:2]), 0)
    with pytest.raises(Nv.NativeError, match=r"0 entry.*\{-1, \+1\}"):
        BucketTable.build(Nv.pack_codes(_t(zero)), 128)
    assert not launched
    monkeypatch.undo()
    index = CodeIndex(_t(rB))
    index.buckets()
    for name in ("bucket_probe_count", "bucket_probe_fill"):
        monkeypatch.setattr(Nv, name, lambda *a, _n=name, **k: launched.append(_n))
    with pytest.raises(Nv.NativeError, match=r"a query with a 0 entry"):
        index.lookup(_t(zero[3:4]), 1)
    with pytest.raises(Nv.NativeError, match=r"radius=3 .*BUCKET_RADIUS_MAX = 2"):
        index.lookup(_t(rB[:2]), 3)
    with pytest.raises(Nv.NativeError, match=r"radius=0.5 .*whole number"):
        index.lookup(_t(rB[:2]), 0.5)
    with pytest.raises(Nv.NativeError, match=r"64-bit queries for an index of 128 bits"):
        index.lookup(_t(rB[:2, :64]), 0)
    with pytest.raises(Nv.NativeError, match=r"query labels given, but the index has none"):
        index.lookup(_t(rB[:2]), 0, torch.ones(2, 4))
    wide = np.concatenate([rB, rB[:, :32]], axis=1)
    with pytest.raises(Nv.NativeError, match=r"160-bit codes exceed BUCKET_BITS_MAX = 128"):
        CodeIndex(_t(wide)).lookup(_t(wide[:2]), 0)
    assert not launched
    monkeypatch.undo()
    assert CodeIndex(_t(wide)).bucket_stats()["distinct"] == torch.unique(_t(rB), dim=0).shape[0]      # the sort takes 160 bits


def test_retrieve_cli_lookup_prints_radius_lines_and_bucket_stats(tmp_path, capsys):
    import scipy.io as scio
    import retrieve
    from utils.code_stats import bucket_summary_lines
    from utils.retrieval import CodeIndex
    rB, rL, qB, qL = U.lookup_case("dense16", 9)
    mat = tmp_path / "codes.mat"
    scio.savemat(str(mat), {"q_img": qB, "q_txt": qB[::-1].copy(), "r_img": rB[::-1].copy(), "r_txt": rB, "q_l": qL, "r_l": rL})
    CodeIndex(_t(rB), _t(rL)).save(tmp_path / "db.npz")
    for extra in ([], ["--index", str(tmp_path / "db.npz")]):
        base = ["--codes", str(mat), "--direction", "i2t", "--queries", "0:7"] + extra
        for radius in ("0", "2"):
            assert retrieve.main(base + ["--radius", radius]) == 0
            want = capsys.readouterr().out
            assert retrieve.main(base + ["--lookup", radius]) == 0
            got = capsys.readouterr().out
            assert got == want and len(got.splitlines()) == 7 and ":" in got
    out = tmp_path / "buckets.npz"
    assert retrieve.main(["--codes", str(mat), "--bucket-stats", "--stats-out", str(out)]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    st = CodeIndex(_t(rB)).bucket_stats()
    assert lines == bucket_summary_lines("r_img", st) + bucket_summary_lines("r_txt", st) and "distinct 137" in lines[0]
    with np.load(out) as z:
        np.testing.assert_array_equal(z["r_txt_bucket_occupancy"], st["occupancy"])
        assert int(z["r_img_bucket_distinct"]) == 137 and int(z["r_img_bucket_collisions"]) == st["collisions"]
    assert retrieve.main(["--index", str(tmp_path / "db.npz"), "--bucket-stats"]) == 0
    assert capsys.readouterr().out.strip().splitlines() == bucket_summary_lines("index", st)
    zero = rB.copy()
    zero[0, 0] = 0
    scio.savemat(str(mat), {"q_img": qB, "q_txt": qB, "r_img": zero, "r_txt": zero, "q_l": qL, "r_l": rL})
    for argv in (["--codes", str(mat), "--lookup", "1"], ["--codes", str(mat), "--bucket-stats"]):
        with pytest.raises(SystemExit, match="0 entry"):
            retrieve.main(argv)


def _state(seed=7):
    import recipe
    return {k: torch.from_numpy(v) for k, v in recipe.clip_state_dict(recipe.CLIP_TINY, seed).items()}


def test_trainer_eval_buckets(tmp_path, monkeypatch):
    """A short DSPH run on the synthetic set (the configuration of the other end-to-end tests), then test() from its checkpoint
    without and with --eval-buckets: the second .mat holds the six usual keys unchanged plus the buckets_ keys, whose tables are
    np.unique's on the stored codes; the log holds the four numbers per side."""
    import argparse
    import scipy.io as scio
    import main
    import dataset.synthetic as ds
    ck = tmp_path / "clip.pt"
    torch.save(_state(), ck)
    monkeypatch.setattr(ds, "SOT", 510); monkeypatch.setattr(ds, "EOT", 511)
    common = ["main.py", "-clip-path", str(ck), "--batch-size", "16", "--num-workers", "0", "--resolution", "64",
              "--max-words", "16", "--query-num", "24", "--train-num", "32", "--synthetic-size", "120", "--gemm-dtype", "f32"]
    monkeypatch.setattr(sys, "argv", common + ["--save-dir", str(tmp_path / "run"), "--epochs", "1"])
    main.trainers["DSPH"](argparse.Namespace(method="DSPH", dataset="synthetic", output_dim=16, is_train=True), 0)
    model = tmp_path / "run" / "DSPH" / "synthetic" / "16" / "model-0.pth"
    assert model.exists()
    runs = {}
    for tag, extra in (("plain", []), ("buckets", ["--eval-buckets", "true"])):
        monkeypatch.setattr(sys, "argv", common + ["--save-dir", str(tmp_path / tag), "--pretrained", str(model)] + extra)
        main.trainers["DSPH"](argparse.Namespace(method="DSPH", dataset="synthetic", output_dim=16, is_train=False), 0)
        path = tmp_path / tag / "DSPH" / "synthetic" / "16" / "PR_cruve" / "16-ours-synthetic-i2t.mat"
        log = open(tmp_path / tag / "DSPH" / "synthetic" / "16" / "test.log").read()
        runs[tag] = ({k: v for k, v in scio.loadmat(path).items() if not k.startswith("__")}, log)
    plain, rec = runs["plain"][0], runs["buckets"][0]
    assert set(plain) == {"q_img", "q_txt", "r_img", "r_txt", "q_l", "r_l"}
    for k in plain:
        np.testing.assert_array_equal(plain[k], rec[k])
    assert set(rec) - set(plain) == {f"buckets_{side}_{what}" for side in ("img", "txt")
                                     for what in ("occupancy", "distinct", "singletons", "largest", "collisions", "collision_probability")}
    for side in ("img", "txt"):
        counts = np.unique(plain[f"r_{side}"], axis=0, return_counts=True)[1]
        sizes, buckets = np.unique(counts, return_counts=True)
        np.testing.assert_array_equal(rec[f"buckets_{side}_occupancy"], np.stack([sizes, buckets], axis=1))
        assert int(rec[f"buckets_{side}_distinct"].ravel()[0]) == counts.size
        assert int(rec[f"buckets_{side}_largest"].ravel()[0]) == counts.max()
        n = plain[f"r_{side}"].shape[0]
        line = (f"buckets({side}): distinct: {counts.size}, singletons: {int((counts == 1).sum())}, largest: {int(counts.max())}, "
                f"collision probability: {float((counts.astype(np.float64) ** 2).sum() / (n * n)):.6e}")
        assert line in runs["buckets"][1]
    assert "buckets(" not in runs["plain"][1]
