"""Host side of the soft-query search, without a GPU: the entry points in the binding and the header, the shape refusals of
csrc/retrieval_soft.hip (they run before any HIP call), the soft rules next to the code rules, and retrieve.py's --soft."""
import os
import re
import subprocess
import sys

import numpy as np

from conftest import PKG, ROOT


def test_entry_points_in_binding_and_header():
    import cmh_native as N
    header = open(os.path.join(ROOT, "include", "cmh.h")).read()
    for name in ("cmh_soft_query_planes", "cmh_soft_topk_workspace_bytes", "cmh_soft_topk"):
        assert name in N.SIGNATURES and re.search(r"\b%s\s*\(" % name, header)
    for name, value in (("CMH_SOFT_LEVELS", N.SOFT_LEVELS), ("CMH_SOFT_Q_MAX", N.SOFT_Q_MAX), ("CMH_SOFT_K_MAX", N.SOFT_K_MAX),
                        ("CMH_SOFT_BITS_MAX", N.SOFT_BITS_MAX)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header)
    assert (N.SOFT_LEVELS, N.SOFT_Q_MAX, N.SOFT_K_MAX, N.SOFT_BITS_MAX) == (15, 64, 4096, 128) and N.ABI_VERSION == 6


def test_workspace_query_and_its_limits():
    import cmh_native as N
    lib = N.lib()
    assert lib.cmh_soft_topk_workspace_bytes(1, 2 ** 31 - 1, 128) > 0 and lib.cmh_soft_topk_workspace_bytes(64, 1, 1) > 0
    for Q, n, bits in ((0, 10, 16), (65, 10, 16), (1, 0, 16), (1, 2 ** 31, 16), (1, 10, 0), (1, 10, 129)):
        assert lib.cmh_soft_topk_workspace_bytes(Q, n, bits) == 0, (Q, n, bits)
    # the images of every legal shape stay under 256 MiB (plus totals and part prefixes: 33 words per (query, bin))
    for Q in (1, 2, 3, 16, 17, 64):
        for n in (1, 4099, 524288, 2_000_000, 2 ** 31 - 1):
            for bits in (1, 64, 128):
                assert 0 < lib.cmh_soft_topk_workspace_bytes(Q, n, bits) <= (256 << 20) + Q * (30 * bits + 1) * 33 * 4 + 1024


def test_limits_are_refused_on_the_host():
    """Nothing is launched: the shape checks run before any HIP call, so they answer without a GPU."""
    import cmh_native as N
    lib = N.lib()
    one = 1       # any non-null address: the arguments are refused before a pointer is read
    for Q, n, bits, k, what in ((65, 100, 16, 5, b"Q=65"), (0, 100, 16, 5, b"Q=0"), (1, 100, 16, 4097, b"k=4097"),
                                (1, 9, 16, 10, b"exceeds N"), (1, 100, 129, 5, b"bits=129"), (1, 100, 16, 0, b"k=0"),
                                (1, 2 ** 31, 16, 5, b"N=2147483648")):
        assert lib.cmh_soft_topk(one, one, one, one, Q, n, bits, k, one, one, one, 1 << 30, None) == -1
        assert what in lib.cmh_last_error(), lib.cmh_last_error()
    for null in range(4):
        ptrs = [None if i == null else one for i in range(4)]
        assert lib.cmh_soft_topk(*ptrs, 1, 100, 16, 5, one, one, one, 1 << 30, None) == -1 and b"null" in lib.cmh_last_error()
    assert lib.cmh_soft_topk(one, one, one, one, 1, 100, 16, 5, None, one, one, 1 << 30, None) == -1
    assert lib.cmh_soft_topk(16, 16, 20, 16, 1, 100, 64, 5, 16, 16, 16, 1 << 30, None) == -1      # rows of 8 bytes at address 20
    assert b"aligned" in lib.cmh_last_error()
    need = lib.cmh_soft_topk_workspace_bytes(1, 100, 16)
    assert lib.cmh_soft_topk(16, 16, 16, 16, 1, 100, 16, 5, 16, 16, 16, need - 1, None) == -2     # one byte short
    assert b"workspace" in lib.cmh_last_error()
    assert lib.cmh_soft_topk(16, 16, 16, 16, 1, 100, 16, 5, 16, 16, None, need, None) == -2
    # the quantiser
    assert lib.cmh_soft_query_planes(None, 1, 16, one, one, one, one, one, None) == -1 and b"null" in lib.cmh_last_error()
    assert lib.cmh_soft_query_planes(one, 1, 16, one, one, one, one, None, None) == -1
    for Q, bits, what in ((0, 16, b"Q=0"), (1, 0, b"bits=0"), (1, 129, b"bits=129")):
        assert lib.cmh_soft_query_planes(one, Q, bits, one, one, one, one, one, None) == -1
        assert what in lib.cmh_last_error()


def test_soft_rules_go_with_the_code_rules():
    import torch

    from code_rules import CODE_RULES, SOFT_RULES, pair_margin, soft_rule
    from query import MODELS
    assert set(SOFT_RULES) == set(CODE_RULES) == set(MODELS)
    assert all(soft_rule(m) is SOFT_RULES[m] for m in SOFT_RULES)
    # the sign methods: the output itself; DNPH: the first output; DCHMT: p1 - p0 of each pair, from the list and from its concatenation
    out = torch.tensor([[0.5, -0.25, 0.0], [-1.0, 1.0, 0.125]])
    for m in ("DSPH", "DNpH", "DMsH_LN", "DHaPH"):
        assert torch.equal(SOFT_RULES[m](out), out)
    assert torch.equal(SOFT_RULES["DNPH"]((out, torch.zeros(2, 7))), out)
    pairs = [torch.tensor([[0.25, 0.75], [0.5, 0.5]]), torch.tensor([[0.875, 0.125], [0.0, 1.0]])]
    want = torch.tensor([[0.5, -0.75], [0.0, 1.0]])
    assert torch.equal(pair_margin(pairs), want) and torch.equal(SOFT_RULES["DCHMT"](torch.cat(pairs, -1)), want)
    # wherever the margin is non-zero its sign is the argmax's code (index 0 -> -1, 1 -> +1; a tie goes to index 0)
    code = torch.cat(pairs, -1).view(2, -1, 2).argmax(-1) * 2 - 1
    assert torch.equal(torch.sign(want)[want != 0], code.float()[want != 0])


def test_restatement_of_the_quantiser():
    """tests/softutil.py itself on values worked out by hand: half-way products round to even, the scale is the largest magnitude."""
    import softutil
    u = np.array([[1.0, 0.5 / 15, 2.5 / 15, 3.5 / 15, -14.5 / 15, 0.0, -0.0, 0.49 / 15],
                  [0.0] * 8,
                  [-2.0, 1.0, -1.0, 0.5, 0.1, -0.1, 0.0, 2.0]], np.float32)
    w, wsum, scale = softutil.quantise(u)
    assert w[1].tolist() == [0] * 8 and wsum[1] == 0 and scale[1] == 0
    assert w[2].tolist() == [-15, 8, -8, 4, 1, -1, 0, 15] and scale[2] == 2.0      # 7.5 -> 8, 3.75 -> 4, 0.75 -> 1
    assert w[0, 0] == 15 and w[0, 5] == 0 and w[0, 6] == 0 and w[0, 7] == 0 and scale[0] == 1.0
    rB = np.array([[1, 1, 1, 1, 1, 1, 1, 1], [0] * 8, [-1, 1, -1, 1, 1, -1, 1, 1]], np.float32)
    d = softutil.wdist(w[2:3], rB)
    assert d.tolist() == [[2 * (15 + 8 + 1), 52, 0]]
    sign, mag = softutil.planes(w[2:3])
    assert sign.tolist() == [[0b10011010]] and mag[0, :, 0].tolist() == [0b10110001, 0b10000001, 0b10001001, 0b10000111]


def _retrieve(*argv):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, os.path.join(PKG, "retrieve.py"), *argv], capture_output=True, text=True, timeout=300, env=env)


def test_retrieve_soft_arguments():
    import retrieve
    model = ["--method", "DSPH", "--pretrained", "m.pth", "-clip-path", "c.pt", "--output-dim", "16"]
    args = retrieve.parse(["--text", "a", "--soft", "--index", "db.npz", *model])
    assert args.soft is True and args.ask == [("text", "a")]
    assert retrieve.parse(["--text", "a", "--index", "db.npz", *model]).soft is False
    assert retrieve.parse(["--codes", "f.mat"]).soft is False
    out = _retrieve("--soft", "--index", "db.npz", *model)                       # no question
    assert out.returncode == 2 and "--soft goes with --text / --image" in out.stderr
    out = _retrieve("--soft", "--codes", "f.mat")
    assert out.returncode == 2 and "--soft goes with --text / --image" in out.stderr
    out = _retrieve("--text", "a", "--soft", "--codes", "f.mat", "--index", "db.npz", *model)
    assert out.returncode == 2 and "exclude each other" in out.stderr
