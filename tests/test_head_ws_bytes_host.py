"""The workspace sizes of the heads and losses, pinned: the eight *_workspace_bytes queries of csrc/losses.hip, heads_bwd.hip, msl.hip, qmi.hip
and mith.hip are pure host arithmetic (a carve_* function over a null base, or the formula two layouts share), so nothing is launched here.
tests/golden/head_ws_bytes.json was recorded from the library of the commit BEFORE the layouts were stated once (csrc/head_common.h: Carver):

    CMH_LIB=<that library> PYTHONPATH=clip-based-cross-modal-hashing_amd python tests/test_head_ws_bytes_host.py
                                                        (writes the file; never run it on the code under test)

Only the totals are pinned here; that every slot kept its place is what tools/heads_ab.py shows on the GPU (bit-identical outputs).  The last
test gives every entry point that takes a workspace one byte less than it needs: the size check sits before the first HIP call of each."""
import ctypes as C
import json
import os

import cmh_native as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_ws_bytes.json")
BS, KS, CS = (1, 3, 63, 64, 65, 256, 1025), (1, 16, 64, 65, 512), (1, 5, 24, 65, 4096)
NCE = ((1, 1), (64, 64), (256, 256), (16384, 64), (130, 65))                      # (R, G)
BAYES_B, BAYES_K = (1, 16, 17, 256), (4, 16, 64, 128)
INVALID, WORKSPACE = -1, -2                                                       # CMH_ERR_INVALID, CMH_ERR_WORKSPACE (include/cmh.h)


def measure():
    lib, out = N.lib(), {}
    for B in BS:
        for K in KS:
            for Cn in CS:
                out[f"loss/b{B}/k{K}/c{Cn}"] = lib.cmh_loss_workspace_bytes(B, K, Cn)
                out[f"head_backward/b{B}/k{K}/c{Cn}"] = lib.cmh_head_backward_workspace_bytes(B, K, Cn)
                out[f"dnph_backward/b{B}/k{K}/c{Cn}"] = lib.cmh_dnph_backward_workspace_bytes(B, K, Cn)
    for B in BS + (8192,):
        out[f"msl/b{B}"] = lib.cmh_msl_workspace_bytes(B)
        out[f"spl/b{B}"] = lib.cmh_spl_workspace_bytes(B)
        out[f"qmi/b{B}"] = lib.cmh_qmi_workspace_bytes(B)
    for R, G in NCE:
        out[f"info_nce/r{R}/g{G}"] = lib.cmh_info_nce_workspace_bytes(R, G)
    for B in BAYES_B:
        for K in BAYES_K:
            out[f"bayesian_backward/b{B}/k{K}"] = lib.cmh_mith_bayesian_backward_workspace_bytes(B, K)
    return out


def test_the_grid_is_the_recorded_one():
    got, want = measure(), json.load(open(GOLDEN))
    assert sorted(got) == sorted(want)
    assert len(got) == 3 * 7 * 5 * 5 + 3 * 8 + 5 + 4 * 4 and all(v > 0 for v in want.values())


def test_workspace_bytes_equal_the_recorded_sizes():
    got, want = measure(), json.load(open(GOLDEN))
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"{len(wrong)} of {len(want)} workspace sizes moved, e.g. {sorted(wrong.items())[:4]}"


def test_queries_refuse_bad_dimensions_with_zero():
    lib = N.lib()
    for q in (lib.cmh_loss_workspace_bytes, lib.cmh_head_backward_workspace_bytes, lib.cmh_dnph_backward_workspace_bytes):
        for dims in ((0, 16, 5), (4, 0, 5), (4, 16, 0), (-1, 16, 5), (4, -16, 5), (4, 16, -5)):
            assert q(*dims) == 0, dims
    for q in (lib.cmh_msl_workspace_bytes, lib.cmh_spl_workspace_bytes, lib.cmh_qmi_workspace_bytes):
        assert q(0) == 0 and q(-7) == 0
    for q in (lib.cmh_info_nce_workspace_bytes, lib.cmh_mith_bayesian_backward_workspace_bytes):
        assert q(0, 4) == 0 and q(4, 0) == 0 and q(-4, 4) == 0 and q(4, -4) == 0


def test_a_workspace_one_byte_short_is_refused_before_any_launch():
    """Every head / loss entry point that takes a workspace, with valid shapes, non-null operands (host addresses the call never reads)
    and need - 1 bytes: the status is the entry's own error class, and nothing was launched, so this runs without a GPU."""
    lib = N.lib()
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    B, K, Cn, M, Nn, R, G, D, Mb = 5, 16, 7, 6, 9, 130, 65, 64, 40
    loss, hbwd, dnph = lib.cmh_loss_workspace_bytes(B, K, Cn), lib.cmh_head_backward_workspace_bytes(B, K, Cn), lib.cmh_dnph_backward_workspace_bytes(B, K, Cn)
    msl, spl, qmi = lib.cmh_msl_workspace_bytes(B), lib.cmh_spl_workspace_bytes(B), lib.cmh_qmi_workspace_bytes(B)
    bayes = lib.cmh_mith_bayesian_backward_workspace_bytes(B, K)
    cases = {   # entry: (expected status, need, call with the workspace size as its argument)
        "dsph_hyp_loss": (WORKSPACE, loss, lambda n: lib.cmh_dsph_hyp_loss(p, p, p, p, B, K, Cn, 0.5, 1.0, p, p, n, None)),
        "dchmt_loss": (WORKSPACE, loss, lambda n: lib.cmh_dchmt_loss(p, p, p, B, K, Cn, 16, 1, 2, 0.5, 0.0, p, p, n, None)),
        "dsph_hyp_loss_backward": (WORKSPACE, hbwd, lambda n: lib.cmh_dsph_hyp_loss_backward(p, p, p, p, B, K, Cn, 0.5, 1.0, p, p, p, p, p, n, None)),
        "dchmt_loss_backward": (WORKSPACE, hbwd, lambda n: lib.cmh_dchmt_loss_backward(p, p, p, B, K, Cn, 16, 1, 2, 0.5, 0.0, p, p, p, p, n, None)),
        "dnph_loss_backward": (WORKSPACE, dnph, lambda n: lib.cmh_dnph_loss_backward(p, p, p, p, p, p, p, p, B, K, Cn, 0.1, 0.5, p, p, p, p, p, p, p, n, None)),
        "linear_act_backward": (WORKSPACE, M * Nn * 4 + 256, lambda n: lib.cmh_linear_act_backward(p, p, p, p, None, 1.0, N.ACT_TANH, p, p, p, M, Nn, K, p, n, None)),
        "twdh_loss": (WORKSPACE, 256, lambda n: lib.cmh_twdh_loss(p, p, p, B, K, p, p, n, None)),
        "dnph_loss": (WORKSPACE, 256, lambda n: lib.cmh_dnph_loss(p, p, p, p, p, p, None, None, B, K, Cn, 0.1, 0.0, p, p, n, None)),
        "sq_diff_sum": (INVALID, 256, lambda n: lib.cmh_sq_diff_sum(p, p, 100, p, p, n, None)),
        "mith_bayesian_loss": (INVALID, 256, lambda n: lib.cmh_mith_bayesian_loss(p, p, p, p, Mb, B, K, Cn, p, p, n, None)),
        "mith_bayesian_loss_backward": (WORKSPACE, bayes, lambda n: lib.cmh_mith_bayesian_loss_backward(p, p, p, p, Mb, B, K, Cn, p, p, p, n, None)),
        "info_nce": (INVALID, 256, lambda n: lib.cmh_info_nce(p, p, R, G, D, 0.07, p, p, n, None)),
        "info_nce_backward": (WORKSPACE, 2 * R * 4 + 256, lambda n: lib.cmh_info_nce_backward(p, p, R, G, D, 0.07, p, p, p, p, n, None)),
        "msl_loss": (WORKSPACE, msl, lambda n: lib.cmh_msl_loss(p, p, p, B, K, Cn, p, p, n, None)),
        "msl_loss_backward": (WORKSPACE, msl, lambda n: lib.cmh_msl_loss_backward(p, p, p, B, K, Cn, p, p, p, p, n, None)),
        "spl_loss": (WORKSPACE, spl, lambda n: lib.cmh_spl_loss(p, p, p, B, K, Cn, 0.3, 0.5, p, p, n, None)),
        "spl_loss_backward": (WORKSPACE, spl, lambda n: lib.cmh_spl_loss_backward(p, p, p, B, K, Cn, 0.3, 0.5, p, p, p, p, n, None)),
        "qmi_loss": (INVALID, qmi, lambda n: lib.cmh_qmi_loss(p, p, p, B, K, Cn, 1e-8, p, p, p, n, None)),
        "qmi_loss_backward": (INVALID, qmi, lambda n: lib.cmh_qmi_loss_backward(p, p, p, B, K, Cn, 1e-8, p, p, p, p, p, n, None)),
    }
    for name, (status, need, call) in cases.items():
        assert need > 0, name
        assert call(need - 1) == status, (name, need, call(need - 1), lib.cmh_last_error())
        assert name.encode() in lib.cmh_last_error(), (name, lib.cmh_last_error())


if __name__ == "__main__":
    sizes = measure()
    with open(GOLDEN, "w") as f:
        json.dump(sizes, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(sizes)} sizes of {N.LIB_PATH} -> {GOLDEN}")
