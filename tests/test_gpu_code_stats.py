"""The code diagnostics on the GPU (cmh_code_gram, utils/code_stats.py, CodeIndex.stats, retrieve.py --stats, the trainers'
--eval-codes) against the NumPy restatement of tests/statsutil.py, which works from the float codes.  Every integer is compared
exactly; the float64 statistics within 1e-12 (host arithmetic on both sides, over the same integers in another order)."""
import sys

import numpy as np
import pytest
import torch

import statsutil as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-12
FILL = 0x5555555555555555

NS = [1, 63, 64, 65, 255, 256, 257, 1000]      # 1000 at 64 items per chunk: 16 chunks, the last of 40 items
SYMMETRIC = [(b, b) for b in (1, 31, 32, 33, 64, 65, 96, 128, 256)]
ASYMMETRIC = [(24, 64), (80, 128), (21, 16), (255, 1), (1, 255)]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _planes(B):
    import cmh_native as N
    return N.pack_codes(_t(B))


def _call(a, b, abits, bbits, chunk=64, sums=True):
    """ONE cmh_code_gram into outputs that hold 0x55 bytes -> the five int64 arrays (the sums None when not asked for)."""
    import cmh_native as N
    lib = N.lib()
    n = a[0].shape[0]
    outs = [torch.full(shape, FILL, dtype=torch.int64, device=DEV) for shape in ((abits, bbits), (abits,), (abits,), (bbits,), (bbits,))]
    if not sums:
        outs[1:] = [None] * 4
    need = lib.cmh_code_gram_workspace_bytes(n, abits, bbits, chunk)
    assert need > 0
    ws = torch.full((need,), 0x55, dtype=torch.uint8, device=DEV)
    N.check(lib.cmh_code_gram(N.ptr(a[0]), N.ptr(a[1]), N.ptr(b[0]), N.ptr(b[1]), n, abits, bbits, chunk, *(N.ptr(t) for t in outs),
                              N.ptr(ws), need, N.stream_ptr(torch.device(DEV))), "cmh_code_gram")
    return [None if t is None else t.cpu().numpy() for t in outs]


def _same(got, want):
    for g, w, name in zip(got, want, ("gram", "a_sum", "a_abs", "b_sum", "b_abs")):
        assert g.dtype == np.int64 and g.shape == w.shape, name
        np.testing.assert_array_equal(g, w, err_msg=name)


@pytest.mark.parametrize("abits,bbits", SYMMETRIC + ASYMMETRIC)
@pytest.mark.parametrize("n", NS)
def test_gram_equals_the_restatement(n, abits, bbits):
    A, B = U.codes(n, abits, n + abits, 0.1), U.codes(n, bbits, n + bbits + 1, 0.1)
    _same(_call(_planes(A), _planes(B), abits, bbits), U.gram(A, B))


@pytest.mark.parametrize("pattern", ["random", "zeros", "plus", "minus", "zero"])
@pytest.mark.parametrize("n,abits,bbits", [(1, 1, 1), (65, 33, 33), (257, 64, 64), (1000, 128, 128), (255, 80, 128), (1000, 21, 16),
                                           (257, 256, 256), (63, 255, 1), (64, 1, 255)])
def test_code_patterns(n, abits, bbits, pattern):
    mk = lambda K, seed: U.codes(n, K, seed, 0.1 if pattern == "zeros" else 0.0, pattern if pattern in ("plus", "minus", "zero") else "random")
    A, B = mk(abits, 3 * n), mk(bbits, 3 * n + 1)
    got = _call(_planes(A), _planes(B), abits, bbits)
    _same(got, U.gram(A, B))
    if pattern in ("plus", "minus"):
        assert (got[0] == n).all() and (np.abs(got[1]) == n).all()
    if pattern == "zero":
        assert not any(g.any() for g in got)


@pytest.mark.parametrize("n,bits", [(65, 33), (1000, 64), (257, 128), (255, 256)])
def test_an_operand_against_itself(n, bits):
    A = U.codes(n, bits, n + bits, 0.1)
    p = _planes(A)
    got = _call(p, p, bits, bits)
    _same(got, U.gram(A, A))
    np.testing.assert_array_equal(got[0], got[0].T)
    np.testing.assert_array_equal(np.diag(got[0]), got[2])
    np.testing.assert_array_equal(got[1], got[3])


@pytest.mark.parametrize("n,C,bits", [(257, 21, 128), (1000, 24, 64), (65, 255, 33), (64, 1, 16)])
def test_label_and_abs_operands(n, C, bits):
    import cmh_native as N
    A, L = U.codes(n, bits, n + C, 0.1), U.labels(n, C, n)
    p, lab = _planes(A), N.pack_labels(_t(L))
    _same(_call((lab, lab), p, C, bits), U.gram(L, A))
    _same(_call((lab, lab), (p[1], p[1]), C, bits), U.gram(L, np.abs(A)))
    _same(_call((p[1], p[1]), p, bits, bits), U.gram(np.abs(A), A))
    gram, cnt = _call((lab, lab), p, C, bits)[:2]
    np.testing.assert_array_equal(cnt, L.sum(0).astype(np.int64))      # a class's size is its label column's sum


@pytest.mark.parametrize("n,abits,bbits", [(257, 33, 65), (1000, 1, 31), (65, 96, 255), (64, 24, 64)])
def test_garbage_above_the_bits_is_ignored(n, abits, bbits):
    A, B = U.codes(n, abits, n, 0.1), U.codes(n, bbits, n + 1, 0.1)
    clean = _call(_planes(A), _planes(B), abits, bbits)
    dirty = []
    for planes, bits in ((_planes(A), abits), (_planes(B), bbits)):
        if bits % 32:
            junk = torch.randint(0, 2 ** 31 - 1, (n,), device=DEV, dtype=torch.int64).to(torch.int32) << (bits % 32)
            planes = tuple(p.clone() for p in planes)
            planes[0][:, -1] |= junk
            planes[1][:, -1] |= junk.flip(0) | (-1 << (bits % 32))      # every bit above `bits` set
        dirty.append(planes)
    _same(_call(dirty[0], dirty[1], abits, bbits), clean)
    _same(clean, U.gram(A, B))


def test_optional_sums_two_calls_and_another_stream():
    n, abits, bbits = 1000, 80, 128
    A, B = U.codes(n, abits, 1, 0.1), U.codes(n, bbits, 2, 0.1)
    a, b = _planes(A), _planes(B)
    first = _call(a, b, abits, bbits)
    _same(first, U.gram(A, B))
    only = _call(a, b, abits, bbits, sums=False)
    np.testing.assert_array_equal(only[0], first[0])
    assert only[1:] == [None] * 4
    for g, w in zip(_call(a, b, abits, bbits), first):
        assert g.tobytes() == w.tobytes()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        other = _call(a, b, abits, bbits)
    for g, w in zip(other, first):
        assert g.tobytes() == w.tobytes()


def test_the_plans_chunks_give_the_forced_chunks_result():
    n, bits = 70000, 64
    A, B = U.codes(n, bits, 5, 0.1), U.codes(n, bits, 6)
    a, b = _planes(A), _planes(B)
    want = U.gram(A, B)
    _same(_call(a, b, bits, bits, chunk=0), want)
    _same(_call(a, b, bits, bits, chunk=64), want)
    _same(_call(a, b, bits, bits, chunk=4096), want)


def test_two_of_the_largest_chunks_and_one_item():
    """The 32-bit partial sums at their largest: all-(+1) codes, so every partial of a full chunk is the chunk's item count."""
    import cmh_native as N
    n = 2 * N.GRAM_CHUNK_MAX + 1
    ones = torch.full((n, 1), -1, dtype=torch.int32, device=DEV)      # 32 bits set in both planes: +1 everywhere
    got = _call((ones, ones), (ones, ones), 32, 32, chunk=N.GRAM_CHUNK_MAX)
    assert all((g == n).all() for g in got)


def _check_stats(got, want, n, K):
    for key in ("bit_mean", "bit_bias", "balance", "bit_entropy", "corr", "mean_abs_corr", "max_abs_corr", "bit_agreement",
                "mean_agreement", "pair_distance", "cross_corr", "class_bit_mean", "bit_class_mi", "best_class_mi"):
        g, w = np.asarray(got[key], dtype=np.float64), np.asarray(want[key], dtype=np.float64)
        assert g.shape == w.shape and float(np.abs(g - w).max()) <= TOL, key
    assert got["dead_bits"] == want["dead_bits"] and got["duplicate_bits"] == want["duplicate_bits"]
    np.testing.assert_array_equal(got["pair_dot"], want["pair_dot"])
    assert got["n"] == n and got["bits"] == K


def test_code_stats_and_index_stats_end_to_end():
    from utils.code_stats import code_stats
    from utils.retrieval import CodeIndex
    n, K, C = 500, 64, 24
    A, B, L = U.codes(n, K, 11, 0.05), U.codes(n, K, 12), U.labels(n, C, 13)
    B[:, :40] = A[:, :40]
    B[::7] = -B[::7]
    A[:, 9], A[:, 17], A[:, 30] = 1.0, A[:, 3], -A[:, 4]            # a dead bit, a copy, a negation
    want = U.stats(A, paired=B, L=L)
    assert want["dead_bits"] == [9] and want["duplicate_bits"] == [(3, 17), (4, 30)] and float(want["live_variance"].min()) >= 0.01
    g, s, ab, _, _ = U.gram(A, A)
    for got in (code_stats(_t(A), labels=_t(L), paired=_t(B)),
                CodeIndex(_t(A), _t(L)).stats(paired=CodeIndex(_t(B))),
                CodeIndex(_t(A), _t(L)).stats(paired=_t(B).cpu())):
        _check_stats(got, want, n, K)
        np.testing.assert_array_equal(got["gram"], g)
        np.testing.assert_array_equal(got["sum"], s)
        np.testing.assert_array_equal(got["abs"], ab)
        np.testing.assert_array_equal(got["pair_gram"], U.gram(A, B)[0])
        np.testing.assert_array_equal(got["class_gram"], U.gram(L, A)[0])
        np.testing.assert_array_equal(got["class_count"], L.sum(0).astype(np.int64))
    alone = CodeIndex(_t(A)).stats()
    assert "bit_agreement" not in alone and "bit_class_mi" not in alone and alone["dead_bits"] == [9]


def test_retrieve_stats(tmp_path, capsys):
    """retrieve.py --stats on a small .mat and on a saved index: the table's numbers are code_stats', the .npz holds the arrays."""
    import scipy.io as scio
    import retrieve
    from utils.code_stats import code_stats, summary_lines
    from utils.retrieval import CodeIndex
    n, K, C = 300, 16, 5
    img, txt, L = U.codes(n, K, 21), U.codes(n, K, 22, 0.1), U.labels(n, C, 23)
    txt[:, :10] = img[:, :10]
    mat, out = tmp_path / "codes.mat", tmp_path / "stats.npz"
    scio.savemat(str(mat), {"q_img": img[:5], "q_txt": txt[:5], "r_img": img, "r_txt": txt, "q_l": L[:5], "r_l": L})
    assert retrieve.main(["--codes", str(mat), "--stats", "--stats-out", str(out)]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    st_img, st_txt = code_stats(_t(img), labels=_t(L), paired=_t(txt)), code_stats(_t(txt), labels=_t(L), paired=_t(img))
    assert lines == summary_lines("r_img", st_img) + summary_lines("r_txt", {k: v for k, v in st_txt.items() if k != "bit_agreement"})
    assert len(lines) == 7 and "pair agreement" in lines[2] and "bit:class:MI" in lines[3]
    with np.load(out) as z:
        np.testing.assert_array_equal(z["r_img_gram"], U.gram(img, img)[0])
        np.testing.assert_array_equal(z["r_txt_pair_gram"], U.gram(txt, img)[0])
        np.testing.assert_array_equal(z["r_img_class_gram"], U.gram(L, img)[0])
        assert float(np.abs(z["r_img_corr"] - U.stats(img)["corr"]).max()) <= TOL
        assert z["r_img_bit_agreement"].shape == (K,) and z["r_txt_bit_class_mi"].shape == (C, K)
    CodeIndex(_t(img), _t(L)).save(tmp_path / "db.npz")
    assert retrieve.main(["--index", str(tmp_path / "db.npz"), "--stats"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines == summary_lines("index", code_stats(_t(img), labels=_t(L)))


def _state(seed=7):
    import recipe
    return {k: torch.from_numpy(v) for k, v in recipe.clip_state_dict(recipe.CLIP_TINY, seed).items()}


def test_trainer_eval_codes(tmp_path, monkeypatch):
    """A short DSPH run on the synthetic set (the configuration of the other end-to-end tests), then test() from its checkpoint
    without and with --eval-codes: the second .mat holds the six usual keys unchanged plus the codes_ keys, whose integers are
    code_gram's on the stored codes and the restatement's; the log holds the three lines."""
    import argparse
    import scipy.io as scio
    import main
    import dataset.synthetic as ds
    from utils.code_stats import code_gram
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
    for tag, extra in (("plain", []), ("codes", ["--eval-codes", "true"])):
        monkeypatch.setattr(sys, "argv", common + ["--save-dir", str(tmp_path / tag), "--pretrained", str(model)] + extra)
        main.trainers["DSPH"](argparse.Namespace(method="DSPH", dataset="synthetic", output_dim=16, is_train=False), 0)
        path = tmp_path / tag / "DSPH" / "synthetic" / "16" / "PR_cruve" / "16-ours-synthetic-i2t.mat"
        log = open(tmp_path / tag / "DSPH" / "synthetic" / "16" / "test.log").read()
        runs[tag] = ({k: v for k, v in scio.loadmat(path).items() if not k.startswith("__")}, log)
    plain, rec = runs["plain"][0], runs["codes"][0]
    assert set(plain) == {"q_img", "q_txt", "r_img", "r_txt", "q_l", "r_l"}
    for k in plain:
        np.testing.assert_array_equal(plain[k], rec[k])
    new = set(rec) - set(plain)
    assert new and all(k.startswith("codes_img_") or k.startswith("codes_txt_") for k in new)
    n, K = plain["r_img"].shape
    for name, other in (("img", "txt"), ("txt", "img")):
        own, oth = plain[f"r_{name}"], plain[f"r_{other}"]
        gram, s, ab = (t.cpu().numpy() for t in code_gram(torch.from_numpy(own).float())[:3])
        np.testing.assert_array_equal(rec[f"codes_{name}_gram"], gram)
        np.testing.assert_array_equal(rec[f"codes_{name}_sum"].ravel(), s)
        np.testing.assert_array_equal(rec[f"codes_{name}_abs"].ravel(), ab)
        np.testing.assert_array_equal(rec[f"codes_{name}_gram"], U.gram(own, own)[0])
        np.testing.assert_array_equal(rec[f"codes_{name}_pair_gram"], U.gram(own, oth)[0])
        np.testing.assert_array_equal(rec[f"codes_{name}_class_gram"], U.gram(plain["r_l"], own)[0])
        assert rec[f"codes_{name}_corr"].shape == (K, K) and rec[f"codes_{name}_bit_agreement"].size == K
        assert int(rec[f"codes_{name}_n"].ravel()[0]) == n
        assert f"codes({name}): balance: " in runs["codes"][1]
    assert "codes(pair): agreement: " in runs["codes"][1] and "codes(" not in runs["plain"][1]
