"""DNPH's noise assignment on the GPU (cmh_assign_rows, csrc/assign.hip) against the reference's own assignments (dnph.npz) and
against the host path (b_reg.gene_noise: numpy cost matrix + scipy), up to the trainer's assign_noise."""
import functools

import numpy as np
import pytest
import torch

from heads2util import DNPH_CASES, dnph_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)

PLAIN = [(1, 16), (2, 16), (3, 8), (63, 32), (64, 64), (65, 64), (129, 64), (256, 64), (256, 128), (300, 128), (512, 64), (1024, 16)]
SATURATED = [(137, 64), (256, 64)]
DUPLICATES = [(40, 4), (64, 5), (137, 6), (256, 8)]
CASES = [("plain", *s) for s in PLAIN] + [("saturated", *s) for s in SATURATED] + [("duplicates", *s) for s in DUPLICATES]


def inputs(kind, B, K):
    """Embeddings: tanh of a Gaussian (saturated: of 6 x the Gaussian, thousands of entries equal to +-1); noise: +-1.  With
    K <= 8 most of the 2^K possible noise rows occur several times."""
    rng = np.random.RandomState(1000 * B + K)
    g = rng.randn(B, K)
    e = np.tanh(g * 6 if kind == "saturated" else g).astype(np.float32)
    s = np.where(rng.randint(0, 2, size=(B, K)) == 0, -1, 1)
    return e, s


@functools.lru_cache(maxsize=None)
def host_case(kind, B, K):
    """The host path's answer, computed once per case: (e, s, cost matrix f64, assigned noise of gene_noise, scipy's optimum)."""
    from scipy.optimize import linear_sum_assignment
    from train.DNPH_TOMM.b_reg import gene_noise
    e, s = inputs(kind, B, K)
    cost = np.linalg.norm(e.astype(np.float64)[:, None, :] - s.astype(np.float64)[None, :, :], axis=2)
    r, c = linear_sum_assignment(cost)
    return e, s, cost, gene_noise(e, s), float(cost[r, c].sum())


@pytest.mark.parametrize("B,K,Cn", DNPH_CASES)
def test_goldens_of_the_reference(golden, B, K, Cn):
    import cmh_native as N
    g = golden("dnph.npz")
    c = dnph_case(B, K, Cn)
    tag = c["tag"]
    s = tt(g[f"{tag}_s_vec"].astype(np.float32))
    emb = torch.stack((tt(c["hi"].astype(np.float32)), tt(c["ht"].astype(np.float32))))
    out = N.assign_rows(emb, s).cpu().numpy()
    assert out.dtype == np.float32
    assert np.array_equal(out[0], g[f"{tag}_noise_i"])
    assert np.array_equal(out[1], g[f"{tag}_noise_t"])


@pytest.mark.parametrize("kind,B,K", CASES)
def test_against_the_host_path(kind, B, K):
    import cmh_native as N
    e, s, cost, want, optimum = host_case(kind, B, K)
    out, col = N.assign_rows(tt(e), tt(s.astype(np.float32)), return_col=True)
    out, col = out.cpu().numpy(), col.cpu().numpy()
    assert col.dtype == np.int32 and sorted(col.tolist()) == list(range(B))                 # a permutation
    assert np.array_equal(out, s[col].astype(np.float32))                                   # the gather is the permutation's
    total = float(cost[np.arange(B), col].sum())                                            # f64, on the host's own cost matrix
    print(f"{kind} {B}x{K}: total {total!r}, scipy {optimum!r}, rel {abs(total - optimum) / optimum:.3e}")
    assert abs(total - optimum) <= 1e-9 * optimum
    assert np.array_equal(out.astype(np.float64), want)                                     # gene_noise's rows


def test_batching_and_determinism():
    import cmh_native as N
    e0, s = inputs("plain", 129, 64)
    rng = np.random.RandomState(5)
    e1 = np.tanh(rng.randn(129, 64)).astype(np.float32)
    e2 = np.tanh(rng.randn(129, 64) * 3).astype(np.float32)
    rows = tt(s.astype(np.float32))
    both, col_both = N.assign_rows(tt(np.stack((e0, e1))), rows, return_col=True)
    singles = [N.assign_rows(tt(e), rows, return_col=True) for e in (e0, e1, e2)]
    for p in range(2):
        assert torch.equal(both[p], singles[p][0]) and torch.equal(col_both[p], singles[p][1])
    three, col_three = N.assign_rows(tt(np.stack((e0, e1, e2))), rows, return_col=True)
    for p in range(3):
        assert torch.equal(three[p], singles[p][0]) and torch.equal(col_three[p], singles[p][1])
    again = N.assign_rows(tt(np.stack((e0, e1, e2))), rows, return_col=True)[1]
    assert torch.equal(again, col_three)


def test_refusals():
    import cmh_native as N
    for B in (1025, 0):
        with pytest.raises(N.NativeError):
            N.assign_rows(torch.zeros(B, 8, device=DEV), torch.ones(B, 8, device=DEV))
    P, B, K = 2, 16, 8
    emb, rows = torch.zeros(P, B, K, device=DEV), torch.ones(B, K, device=DEV)
    out = torch.empty(P, B, K, device=DEV)
    need = N.lib().cmh_assign_rows_workspace_bytes(P, B)
    assert need >= P * B * B * 8 + P * B * 4
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    call = lambda nbytes: N.lib().cmh_assign_rows(N.ptr(emb), N.ptr(rows), P, B, K, N.ptr(out), None, N.ptr(ws), nbytes, N.stream_ptr(DEV))
    with pytest.raises(N.NativeError):
        N.check(call(need - 1), "cmh_assign_rows")
    N.check(call(need), "cmh_assign_rows")
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,K", [(9, 16), (256, 64)])
def test_trainer_paths_agree(B, K):
    from train.DNPH_TOMM.b_reg import assign_noise, rand_unit_rect
    rng = np.random.RandomState(B + K)
    hi, ht = tt(np.tanh(rng.randn(B, K)).astype(np.float32)), tt(np.tanh(rng.randn(B, K)).astype(np.float32))
    got = {}
    for how in ("gpu", "host"):
        np.random.seed(1814)
        got[how] = assign_noise(hi.clone().requires_grad_(), ht.clone().requires_grad_(), rand_unit_rect(B, K), how)
    for a, b in zip(got["gpu"], got["host"]):
        assert a.dtype == b.dtype == torch.float32 and a.is_cuda and b.is_cuda and not a.requires_grad
        assert a.shape == (B, K) and torch.equal(a, b)


def test_gpu_path_makes_no_host_trip(monkeypatch):
    from train.DNPH_TOMM.b_reg import assign_noise, rand_unit_rect
    rng = np.random.RandomState(3)
    hi, ht = tt(np.tanh(rng.randn(40, 32)).astype(np.float32)), tt(np.tanh(rng.randn(40, 32)).astype(np.float32))
    np.random.seed(7)
    s = rand_unit_rect(40, 32)
    want = assign_noise(hi, ht, s, "host")

    def refuse(*a, **k):
        raise AssertionError("the gpu path went to the host")
    with monkeypatch.context() as m:
        for name in ("cpu", "numpy", "item", "tolist"):
            m.setattr(torch.Tensor, name, refuse)
        with pytest.raises(AssertionError):
            assign_noise(hi, ht, s, "host")                 # the patch bites
        got = assign_noise(hi, ht, s, "gpu")
        torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
