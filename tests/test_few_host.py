"""Host side of the few-query search and the query front end, without a GPU: the entry points in the binding and the header, the
routing rule of utils/retrieval.py, the refusals of retrieve.py's query mode and of QueryEncoder."""
import os
import re
import subprocess
import sys

import pytest

from conftest import PKG, ROOT


def test_entry_points_in_binding_and_header():
    import cmh_native as N
    header = open(os.path.join(ROOT, "include", "cmh.h")).read()
    for name in ("cmh_hamming_topk_few", "cmh_topk_few_workspace_bytes"):
        assert name in N.SIGNATURES and re.search(r"\b%s\s*\(" % name, header)
    for name, value in (("CMH_FEW_Q_MAX", N.FEW_Q_MAX), ("CMH_FEW_K_MAX", N.FEW_K_MAX), ("CMH_FEW_BITS_MAX", N.FEW_BITS_MAX)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header)
    assert (N.FEW_Q_MAX, N.FEW_K_MAX, N.FEW_BITS_MAX) == (64, 4096, 128) and N.ABI_VERSION == 6


def test_limits_are_refused_on_the_host():
    """Nothing is launched: the shape checks run before any HIP call, so they answer without a GPU."""
    import cmh_native as N
    lib = N.lib()
    assert lib.cmh_topk_few_workspace_bytes(1, 2 ** 31 - 1, 128) > 0 and lib.cmh_topk_few_workspace_bytes(64, 1, 1) > 0
    for Q, n, bits in ((0, 10, 16), (65, 10, 16), (1, 0, 16), (1, 2 ** 31, 16), (1, 10, 0), (1, 10, 129)):
        assert lib.cmh_topk_few_workspace_bytes(Q, n, bits) == 0
    # the images of every legal shape stay under 256 MiB
    for Q in (1, 16, 17, 64):
        for n in (1, 4099, 524288, 2_000_000, 2 ** 31 - 1):
            for bits in (1, 64, 128):
                assert lib.cmh_topk_few_workspace_bytes(Q, n, bits) <= 256 << 20
    one = 1       # any non-null address: the arguments are refused before a pointer is read
    for Q, n, bits, k, what in ((65, 100, 16, 5, b"Q=65"), (1, 100, 16, 4097, b"k=4097"), (1, 9, 16, 10, b"exceeds N"),
                                (1, 100, 129, 5, b"bits=129"), (1, 100, 16, 0, b"k=0")):
        assert lib.cmh_hamming_topk_few(one, one, one, one, Q, n, bits, k, one, one, one, 1 << 30, None) == -1
        assert what in lib.cmh_last_error()
    assert lib.cmh_hamming_topk_few(None, one, one, one, 1, 100, 16, 5, one, one, one, 1 << 30, None) == -1
    assert lib.cmh_hamming_topk_few(16, 16, 16, 16, 1, 100, 16, 5, 16, 16, 16, 8, None) == -2      # workspace too small


def test_few_route_truth_table(monkeypatch):
    from utils import retrieval as R
    assert 0 <= R.QUERIES_FEW <= 64
    monkeypatch.setattr(R, "QUERIES_FEW", 8)
    ok = dict(Q=8, k=4096, bits=128, shard_items=None, graded=False, want_counts=False)
    assert R._few_route(**ok) is True and R._few_route(**dict(ok, Q=1, k=1, bits=1)) is True
    for change in (dict(Q=9), dict(k=4097), dict(bits=129), dict(graded=True), dict(want_counts=True), dict(shard_items=1000),
                   dict(shard_items=524287)):
        assert R._few_route(**dict(ok, **change)) is False, change
    monkeypatch.setattr(R, "QUERIES_FEW", 0)                       # nothing routes to the kernel
    assert R._few_route(**dict(ok, Q=1)) is False
    monkeypatch.setattr(R, "QUERIES_FEW", 1000)                    # never past what the kernel takes
    assert R._few_route(**dict(ok, Q=64)) is True and R._few_route(**dict(ok, Q=65)) is False


def _retrieve(*argv):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, os.path.join(PKG, "retrieve.py"), *argv], capture_output=True, text=True, timeout=300, env=env)


def test_retrieve_argument_refusals():
    model = ["--method", "DSPH", "--pretrained", "m.pth", "-clip-path", "c.pt", "--output-dim", "16"]
    out = _retrieve("--text", "a dog on a beach", *model)
    assert out.returncode == 2 and "--index FILE is required" in out.stderr
    out = _retrieve("--k", "5")
    assert out.returncode == 2 and "the following arguments are required: --codes" in out.stderr
    out = _retrieve("--image", "x.jpg", "--index", "db.npz", "--method", "DSPH")
    assert out.returncode == 2 and "--pretrained" in out.stderr and "--output-dim" in out.stderr
    out = _retrieve("--text", "a", "--index", "db.npz", "--codes", "f.mat", *model)
    assert out.returncode == 2 and "exclude each other" in out.stderr
    import retrieve
    args = retrieve.parse(["--text", "one", "--image", "p.jpg", "--text", "two", "--index", "db.npz", "--k", "3", *model])
    assert args.ask == [("text", "one"), ("image", "p.jpg"), ("text", "two")] and args.k == 3 and args.clip_path == "c.pt"
    assert retrieve.parse(["--codes", "f.mat"]).ask == []


@pytest.mark.parametrize("method", ["MITH", "TwDH"])
def test_query_encoder_refuses_by_name(method, monkeypatch):
    import torch
    from query import QueryEncoder
    boom = lambda *a, **k: (_ for _ in ()).throw(AssertionError("the refusal comes before any GPU work"))
    monkeypatch.setattr(torch.cuda, "current_device", boom)
    monkeypatch.setattr(torch, "load", boom)
    with pytest.raises(NotImplementedError, match=method):
        QueryEncoder(method, "no-such-file.pth", "no-such-clip.pt", 64)
    with pytest.raises(ValueError, match="unknown method"):
        QueryEncoder("NoSuchMethod", "no-such-file.pth", "no-such-clip.pt", 64)
    from code_rules import CODE_RULES
    from query import MODELS
    assert set(CODE_RULES) == set(MODELS)                          # every method the encoder builds has its rule, and no other
