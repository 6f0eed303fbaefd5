"""The soft-query search (csrc/retrieval_soft.hip: cmh_soft_query_planes, cmh_soft_topk) against the NumPy restatement of
tests/softutil.py (the quantiser in np.float32, wdist = sum |w| - r . w, a stable argsort), and against N.hamming_topk_few where the
two must agree.  Integers throughout: every comparison is torch.equal.  Then the Python layers, the query encoder and the command
line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rankutil
import softutil
from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _planes(B):
    import cmh_native as N
    return N.pack_codes(_t(B))


def _check(u, rB, ks, rp=None):
    """soft_topk == NumPy for every k of ks on one pair (soft queries, code matrix); the quantiser's outputs on the way."""
    import cmh_native as N
    bits = u.shape[1]
    q = N.soft_query_planes(_t(u))
    w, wsum, scale = softutil.quantise(u)
    sign, mag = softutil.planes(w)
    assert torch.equal(q[0], _t(sign)) and torch.equal(q[1], _t(mag))
    assert torch.equal(q[2], _t(wsum.astype(np.int32))) and torch.equal(q[3], _t(scale))
    rp = _planes(rB) if rp is None else rp
    for k in ks:
        idx, wd = N.soft_topk(q, rp, bits, k)
        assert idx.dtype == torch.int32 and wd.dtype == torch.int32 and tuple(idx.shape) == tuple(wd.shape) == (u.shape[0], k)
        want_idx, want_wd, _ = softutil.topk(u, rB, k)
        assert torch.equal(idx, _t(want_idx)), (u.shape, rB.shape, k)
        assert torch.equal(wd, _t(want_wd)), (u.shape, rB.shape, k)
    return q, rp


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
def test_edges_of_the_item_walk(n):
    """One item, around a wave, one past a 256-item set of slabs, several ragged chunks; query counts on both sides of every group
    size a workgroup may hold (1, 2, 4, 8, 16); k = 1, 7 and the whole page."""
    _, rB = rankutil.codes(1, n, 64, 0.1, 1000 + n)
    rp = _planes(rB)
    for Q in (1, 2, 3, 4, 5, 8, 9, 16, 17, 64):
        _check(softutil.queries(Q, 64, 7 * n + Q), rB, sorted({1, min(7, n), min(n, 4096)}), rp)


@pytest.mark.parametrize("bits", [16, 32, 33, 64, 96, 128])
def test_code_widths_and_the_cut_of_the_last_word(bits):
    """1..4 words per plane, and 33 bits: one bit in the second word.  Then every bit at and behind `bits` set in both database
    planes and in copies of the query planes: nothing of it may be counted."""
    import cmh_native as N
    _, rB = rankutil.codes(1, 4099, bits, 0.1, 2000 + bits)
    u = softutil.queries(5, bits, 2100 + bits)
    q, (rs, rn) = _check(u, rB, [1, 7, 4096])
    if bits % 32:
        high = torch.tensor(-(1 << (bits % 32)), dtype=torch.int32, device=DEV)        # the bits at and above `bits` of the last word
        rs, rn, qs, qm = rs.clone(), rn.clone(), q[0].clone(), q[1].clone()
        rs[:, -1] |= high
        rn[:, -1] |= high
        qs[:, -1] |= high
        qm[:, :, -1] |= high
        for k in (1, 7, 4096):
            idx, wd = N.soft_topk((qs, qm), (rs, rn), bits, k)
            want_idx, want_wd, _ = softutil.topk(u, rB, k)
            assert torch.equal(idx, _t(want_idx)) and torch.equal(wd, _t(want_wd))


@pytest.mark.parametrize("db_zeros", [0, 0.1])
def test_equals_the_hamming_search_where_it_must(db_zeros):
    """u in {-c, +c}^K: every weight is +-15, so the order is the Hamming order of sign(u) and wdist = 15 h; with zeros in u the
    zero bits leave the distance: wdist = 15 (h - zeros of the query), the same order."""
    import cmh_native as N
    rng = np.random.default_rng(31)
    qB, _ = rankutil.codes(5, 1, 64, 0, 3000)                            # zero-free query codes
    _, rB = rankutil.codes(1, 4099, 64, db_zeros, 3001 + int(10 * db_zeros))
    rp = _planes(rB)
    for c in (0.25, 1.0, 3e-5):
        u = (qB * np.float32(c)).astype(np.float32)
        for k in (1, 7, 4096):
            idx, wd = N.soft_topk(N.soft_query_planes(_t(u)), rp, 64, k)
            f_idx, f_dist = N.hamming_topk_few(_planes(qB), rp, 64, k)
            assert torch.equal(idx, f_idx) and torch.equal(wd, (30 * f_dist).to(torch.int32))      # 15 h = 30 * (h / 2)
    qz = qB.copy()
    qz[rng.random(qz.shape) < 0.2] = 0.0
    qz[:, 0] = 1.0                                                       # (no all-zero row here)
    zeros = _t((qz == 0).sum(1).astype(np.int32))
    for k in (1, 7, 4096):
        idx, wd = N.soft_topk(N.soft_query_planes(_t(0.5 * qz)), rp, 64, k)
        f_idx, f_dist = N.hamming_topk_few(_planes(qz), rp, 64, k)
        assert torch.equal(idx, f_idx) and torch.equal(wd, 15 * ((2 * f_dist).to(torch.int32) - zeros[:, None]))


def test_extremes_of_the_bins():
    """128 bit, all |w| = 15: an item equal to sign(u) lies in bin 0, its negation in the last bin 3840, an all-zero item in bin
    1920; the three at items 0, 255, 256 and n - 1 in turn.  An all-zero u: everything at 0, the answer is 0..k-1.  A u with one
    non-zero entry: two or three bins."""
    import cmh_native as N
    n = 4099
    qB, rB = rankutil.codes(4, n, 128, 0.1, 41)
    u = (0.7 * qB).astype(np.float32)
    u[u == 0] = 0.7                                                      # (rankutil.codes with zeros: make every |w| 15)
    code = np.sign(u)
    for turn, spots in enumerate(((0, 255, 256), (255, 256, n - 1), (256, n - 1, 0), (n - 1, 0, 255))):
        r = rB.copy()
        r[spots[0]], r[spots[1]], r[spots[2]] = code[turn], -code[turn], 0.0
        rp = _planes(r)
        _check(u, r, [4096], rp)
        idx, wd = N.soft_topk(N.soft_query_planes(_t(u[turn:turn + 1])), rp, 128, 1)
        assert idx.tolist() == [[spots[0]]] and wd.tolist() == [[0]]
        full = softutil.wdist(softutil.quantise(u[turn:turn + 1])[0], r)[0]
        assert full[spots[0]] == 0 and full[spots[1]] == 3840 and full[spots[2]] == 1920
    # the far end of the ranking needs the last bin: a database of three items, all of them asked for
    three = np.stack([-code[0], np.zeros(128, np.float32), code[0]])
    idx, wd = N.soft_topk(N.soft_query_planes(_t(u[:1])), _planes(three), 128, 3)
    assert idx.tolist() == [[2, 1, 0]] and wd.tolist() == [[0, 1920, 3840]]
    zero = np.zeros((2, 128), np.float32)
    zero[1, 5] = -0.0
    for k in (1, 4096):
        idx, wd = N.soft_topk(N.soft_query_planes(_t(zero)), _planes(rB), 128, k)
        assert torch.equal(idx, torch.arange(k, dtype=torch.int32, device=DEV).expand(2, k)) and int(wd.abs().max()) == 0
    one = np.zeros((3, 128), np.float32)
    one[0, 0], one[1, 127], one[2, 64] = 0.3, -2.0, 1e-30
    _check(one, rB, [1, 7, 4096])


def test_ties_across_chunks():
    """4099 identical database codes: indices 0..k-1 at one distance; 16-bit codes on 4099 items: tie groups of hundreds, so the
    cut inside the group at the radius falls across chunk boundaries."""
    import cmh_native as N
    _, rB = rankutil.codes(1, 4099, 16, 0, 51)
    u = softutil.queries(5, 16, 52)
    _check(u, rB, [1, 4, 5, 300, 1000, 4096])
    same = np.repeat(rB[7:8], 4099, 0)
    q = N.soft_query_planes(_t(u))
    d = softutil.wdist(softutil.quantise(u)[0], same[:1])[:, 0]
    for k in (1, 257, 4096):
        idx, wd = N.soft_topk(q, _planes(same), 16, k)
        assert torch.equal(idx, torch.arange(k, dtype=torch.int32, device=DEV).expand(5, k))
        assert torch.equal(wd, _t(d.astype(np.int32))[:, None].expand(5, k))


def test_many_chunks():
    _, rB = rankutil.codes(1, 70001, 64, 0.1, 61)
    _check(softutil.queries(3, 64, 62), rB, [1000])


def test_past_one_tiles_call():
    """1 200 000 items at 64 bit in one call: codes drawn on the GPU, the oracle on the host."""
    import cmh_native as N
    g = torch.Generator(device=DEV).manual_seed(71)
    n, bits = 1_200_000, 64
    rB = (torch.randint(0, 3, (n, bits), device=DEV, generator=g) - 1).float()
    u = softutil.queries(3, bits, 72)
    idx, wd = N.soft_topk(N.soft_query_planes(_t(u)), N.pack_codes(rB), bits, 100)
    want_idx, want_wd, _ = softutil.topk(u, rB.cpu().numpy(), 100)
    assert torch.equal(idx, _t(want_idx)) and torch.equal(wd, _t(want_wd))


def _f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def test_quantiser_bit_for_bit():
    """Against the np.float32 restatement: products that land half-way (0.5, 2.5, 3.5, 14.5: round to even), a denormal scale, a
    scale next to the largest float, negative zero, a row whose maximum is negative, rows of other lengths."""
    import cmh_native as N
    rng = np.random.default_rng(81)
    K = 64
    rows = []
    grid = np.array([0.5, 2.5, 3.5, 14.5, 1.5, 7.5, -0.5, -2.5, -14.5, 15.0, 0.0, -0.0, 4.0, 7.0, 11.25, -13.75], np.float32)
    for s in (1.0, 15.0, 30.0, 0.75, 3.0e38 / 15, 1.0e-30):            # u = grid * (s / 15): s = 15, 30 give exact half-way products
        row = np.zeros(K, np.float32)
        row[:16] = grid * np.float32(s / 15)
        row[16:32] = -row[:16]
        rows.append(row)
    den = np.zeros(K, np.float32)                                        # a denormal scale: s = 30 * 2^-149, entries of whole denormals
    den[:31] = _f32(np.arange(31, dtype=np.uint32))
    den[31] = -_f32([30])[0]
    rows.append(den)
    big = rng.uniform(-3e38, 3e38, K).astype(np.float32)
    big[3] = 3e38
    rows.append(big)
    neg = -np.abs(softutil.queries(1, K, 82)[0]) - np.float32(0.01)     # the maximum of the row is negative: the scale is max |u|
    rows.append(neg)
    rows.append(np.where(rng.random(K) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32))      # zeros of both signs: s == 0
    rows.extend(softutil.queries(40, K, 83))
    u = np.stack(rows)
    w, wsum, scale = softutil.quantise(u)
    product = ((u[1] / scale[1]).astype(np.float32) * np.float32(15)).astype(np.float32)      # the row of s = 15: exact half-way products
    assert {0.5, 2.5, 3.5, 14.5, -0.5, -14.5}.issubset(set(product.tolist())) and {0, 2, 4, 14}.issubset(set(np.abs(w[1]).tolist()))
    assert scale[6] == _f32([30])[0] and wsum[9] == 0 and scale[8] > 0 and u[8].max() < 0
    for bits, uu in ((K, u), (33, u[:, :33].copy()), (128, np.concatenate([u, u[:, ::-1]], 1)), (1, u[:, 3:4].copy())):
        w, wsum, scale = softutil.quantise(uu)
        sign, mag = softutil.planes(w)
        qs, qm, qw, qsc = N.soft_query_planes(_t(uu))
        assert torch.equal(qs, _t(sign)) and torch.equal(qm, _t(mag)), bits
        assert torch.equal(qw, _t(wsum.astype(np.int32))) and torch.equal(qsc.view(torch.int32), _t(scale.view(np.int32))), bits
    for poison in (np.nan, np.inf, -np.inf):
        bad = u[:5].copy()
        bad[3, 40] = poison
        with pytest.raises(N.NativeError, match="finite"):
            N.soft_query_planes(_t(bad))


def test_two_calls_give_equal_bytes_on_any_stream():
    import cmh_native as N
    _, rB = rankutil.codes(1, 70001, 32, 0.1, 91)
    q, rp = N.soft_query_planes(_t(softutil.queries(5, 32, 92))), _planes(rB)
    a = N.soft_topk(q, rp, 32, 1000)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b = N.soft_topk(q, rp, 32, 1000)
    s.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_refusals():
    import cmh_native as N
    assert (N.SOFT_Q_MAX, N.SOFT_K_MAX, N.SOFT_BITS_MAX) == (64, 4096, 128)
    _, rB = rankutil.codes(1, 5000, 64, 0, 101)
    rp = _planes(rB)
    q = N.soft_query_planes(_t(softutil.queries(65, 64, 102)))
    with pytest.raises(N.NativeError, match="Q=65"):
        N.soft_topk(q, rp, 64, 10)
    q1 = (q[0][:1], q[1][:1])
    with pytest.raises(N.NativeError, match="k=4097"):
        N.soft_topk(q1, rp, 64, 4097)
    with pytest.raises(N.NativeError, match="exceeds N"):
        N.soft_topk(q1, tuple(x[:9] for x in rp), 64, 10)
    z = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=DEV)
    with pytest.raises(N.NativeError, match="bits=129"):
        N.soft_topk((z(1, 5), z(1, 4, 5)), (z(50, 5), z(50, 5)), 129, 10)
    with pytest.raises(N.NativeError, match="bits=129"):
        N.soft_query_planes(torch.zeros(1, 129, device=DEV))
    for k in (0, -3, 2 ** 40):                                     # refused on the host, before Q x k entries are allocated
        with pytest.raises(N.NativeError, match="k="):
            N.soft_topk(q1, rp, 64, k)
    with pytest.raises(N.NativeError):                             # a query plane of another shape
        N.soft_topk((q[0][:1], q[1][:1, :3]), rp, 64, 10)
    # database planes whose rows of 8 bytes start at an address that is 4 mod 8
    off = [torch.empty(5000 * 2 + 1, dtype=torch.int32, device=DEV)[1:].view(5000, 2).copy_(x) for x in rp]
    assert off[0].data_ptr() % 8 == 4 and off[0].is_contiguous()
    with pytest.raises(N.NativeError, match="aligned"):
        N.soft_topk(q1, tuple(off), 64, 10)
    # a workspace one byte short, natively
    need = N.lib().cmh_soft_topk_workspace_bytes(1, 5000, 64)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    idx, wd = z(1, 10), z(1, 10)
    args = (N.ptr(q1[0]), N.ptr(q1[1]), N.ptr(rp[0]), N.ptr(rp[1]), 1, 5000, 64, 10, N.ptr(idx), N.ptr(wd), N.ptr(ws))
    assert N.lib().cmh_soft_topk(*args, need - 1, N.stream_ptr(ws.device)) == -2
    assert N.lib().cmh_soft_topk(*args, need, N.stream_ptr(ws.device)) == 0
    want = N.soft_topk(q1, rp, 64, 10)
    assert torch.equal(idx, want[0]) and torch.equal(wd, want[1])
    N.soft_topk(q1, rp, 64, 4096)                                  # the limits themselves are legal
    N.soft_topk((q[0][:64], q[1][:64]), rp, 64, 1)


def test_python_layers():
    """CodeIndex.search_soft with 130 queries = its three blocks searched alone; dist is the np.float32 expression; soft_topk on
    code matrices gives the same; another code length, bits > 128 and k > 4096 are refused by name."""
    import cmh_native as N
    from utils import retrieval as R
    _, rB = rankutil.codes(1, 4099, 32, 0.1, 111)
    u = softutil.queries(130, 32, 112)
    index = R.CodeIndex(torch.from_numpy(rB))
    idx, dist, wd = index.search_soft(torch.from_numpy(u), 20)
    assert tuple(idx.shape) == (130, 20) and dist.dtype == torch.float32 and wd.dtype == torch.int32
    for a, b in ((0, 64), (64, 128), (128, 130)):
        part = N.soft_topk(N.soft_query_planes(_t(u[a:b])), index.planes, 32, 20)
        assert torch.equal(idx[a:b], part[0]) and torch.equal(wd[a:b], part[1])
    want_idx, want_wd, want_dist = softutil.topk(u, rB, 20)
    assert torch.equal(idx, _t(want_idx)) and torch.equal(wd, _t(want_wd)) and torch.equal(dist, _t(want_dist))
    again = R.soft_topk(torch.from_numpy(u), torch.from_numpy(rB), 20)
    assert all(torch.equal(x, y) for x, y in zip(again, (idx, dist, wd)))
    one = index.search_soft(torch.from_numpy(u[5]), 3)               # a single row
    assert torch.equal(one[0], idx[5:6, :3])
    with pytest.raises(N.NativeError, match="32 bits"):
        index.search_soft(torch.from_numpy(softutil.queries(2, 64, 113)), 5)
    with pytest.raises(N.NativeError, match="4096"):
        index.search_soft(torch.from_numpy(u[:2]), 4097)
    wide = R.CodeIndex(torch.ones(10, 160))
    with pytest.raises(N.NativeError, match="128"):
        wide.search_soft(torch.ones(1, 160), 5)


# ---- the query encoder and the command line, with tiny models built as tests/test_gpu_query.py builds them --------------------------
MERGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_bpe_merges_48894.txt.gz")
CAPTIONS = ["a dog on a beach", "two people riding bicycles past a red house", "", "a plate of food, with a fork!"]
BITS, WORDS, RES = 16, 16, 64


def _images():
    rng = np.random.default_rng(5)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((64, 64), (48, 80), (33, 257))]


@pytest.fixture(scope="module")
def clip_file(tmp_path_factory):
    import recipe
    sd = recipe.clip_state_dict(dict(recipe.CLIP_TINY, vocab_size=49408), 7)
    path = tmp_path_factory.mktemp("soft") / "clip.pt"
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, path)
    return str(path)


def _checkpoint(method, clip_file, tmp_path):
    import importlib

    from query import MODELS
    module, name = MODELS[method]
    torch.manual_seed(11)
    kw = dict(outputDim=BITS, clipPath=clip_file, saveDir=str(tmp_path / "log"))
    if method == "DNPH":
        kw["num_classes"] = 24
    model = getattr(importlib.import_module(module), name)(**kw).to(DEV)
    ck = tmp_path / f"{method}.pth"
    torch.save(model.state_dict(), ck)
    return str(ck)


@pytest.mark.parametrize("method", ["DSPH", "DCHMT", "DNPH"])
def test_encoder_soft_output_goes_with_its_codes(method, clip_file, tmp_path):
    from query import QueryEncoder
    from utils.retrieval import CodeIndex
    enc = QueryEncoder(method, _checkpoint(method, clip_file, tmp_path), clip_file, BITS, max_words=WORDS, resolution=RES, bpe_path=MERGES)
    g = torch.Generator().manual_seed(3)
    index = CodeIndex((torch.randint(0, 2, (300, BITS), generator=g) * 2 - 1).float())
    for soft, codes in ((enc.encode_text(CAPTIONS, soft=True), enc.encode_text(CAPTIONS)),
                        (enc.encode_image(_images(), soft=True), enc.encode_image(_images())),
                        (enc.encode_tokens(enc.tokenize(CAPTIONS), soft=True), enc.encode_tokens(enc.tokenize(CAPTIONS)))):
        assert tuple(soft.shape) == tuple(codes.shape) == (codes.shape[0], BITS) and soft.dtype == torch.float32
        assert bool(torch.isfinite(soft).all()) and bool((soft != 0).any())
        assert torch.equal(torch.sign(soft)[soft != 0], codes[soft != 0])
        idx, dist, wd = index.search_soft(soft, 10)
        want = softutil.topk(soft.cpu().numpy(), index_codes(index), 10)
        assert torch.equal(idx, _t(want[0])) and torch.equal(wd, _t(want[1])) and torch.equal(dist, _t(want[2]))


def index_codes(index):
    import cmh_native as N
    return N.unpack_codes(*index.planes, index.bits).cpu().numpy()


def test_retrieve_soft_end_to_end(clip_file, tmp_path):
    from PIL import Image

    from query import QueryEncoder
    from utils.retrieval import CodeIndex
    ck = _checkpoint("DSPH", clip_file, tmp_path)
    enc = QueryEncoder("DSPH", ck, clip_file, BITS, max_words=WORDS, resolution=RES, bpe_path=MERGES)
    g = torch.Generator().manual_seed(3)
    CodeIndex((torch.randint(0, 2, (300, BITS), generator=g) * 2 - 1).float()).save(tmp_path / "db.npz")
    picture = tmp_path / "p.png"
    Image.fromarray(_images()[1]).save(picture)
    model = ["--method", "DSPH", "--pretrained", ck, "-clip-path", clip_file, "--output-dim", str(BITS), "--max-words", str(WORDS),
             "--resolution", str(RES), "--bpe-path", MERGES]
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(PKG, "retrieve.py"), "--text", CAPTIONS[0], "--image", str(picture), "--soft",
                          "--index", str(tmp_path / "db.npz"), "--k", "10", *model], capture_output=True, text=True, timeout=600,
                         env=env, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 2 * 11
    soft = torch.cat([enc.encode_text(CAPTIONS[0], soft=True), enc.encode_image(str(picture), soft=True)])
    idx, dist, _ = (t.cpu().numpy() for t in CodeIndex.load(tmp_path / "db.npz").search_soft(soft, 10))
    for i, (kind, value) in enumerate((("text", CAPTIONS[0]), ("image", str(picture)))):
        block = lines[11 * i:11 * i + 11]
        assert block[0] == f"query {i} {kind}: {value}"
        rows = [ln.split() for ln in block[1:]]
        assert [int(r[0]) for r in rows] == list(range(1, 11)) and [int(r[1]) for r in rows] == idx[i].tolist()
        assert [float(r[2]) for r in rows] == [float(f"{d:g}") for d in dist[i]]
