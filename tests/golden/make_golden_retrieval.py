#!/usr/bin/env python3
"""Golden generator of tests/golden/retrieval.npz: top-k Hamming search and distance histograms by relevance.

Distances and relevance are the REFERENCE's own functions, utils/calc_utils.py::calc_hammingDist and calc_neighbor, loaded from a
checkout of the reference (never copied): `python make_golden_retrieval.py <reference checkout>`.  The one thing added here is the
documented ordering, torch.sort(hamm, stable=True) (ties by ascending database index).  Only arrays are written: per case the
inputs (codes int8, labels uint8, k) and idx / dist / rel of the first k columns plus counts[q, h, rel] over half-distances
h = 2 * dist.

Cases: 16 / 64 / 128-bit codes, 48 bit (a partial word) and 512 bit; zeros in the codes of both sides, of the queries only, of the
database only (half-integer distances); N = 1000, 4097, 513 (no multiple of a tile); k = 1, k = N; a query without a relevant item
(query 1 of every labelled case); duplicate codes (every distance 0); 40 classes (two label words); a tie group that straddles the
k boundary with k - count(< h*) = 1 (`tie_one`) and one that is taken whole (`tie_whole`), both for query 0."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def reference_functions(ref):
    spec = importlib.util.spec_from_file_location("ref_calc_utils", os.path.join(ref, "utils", "calc_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.calc_hammingDist, mod.calc_neighbor


def codes(rng, n, bits, zeros):
    vals = np.array([-1, 1, 0] if zeros else [-1, 1], np.int8)
    p = [0.45, 0.45, 0.10] if zeros else [0.5, 0.5]
    return rng.choice(vals, size=(n, bits), p=p)


def labels(rng, n, classes, p=0.12):
    return (rng.random((n, classes)) < p).astype(np.uint8)


def expected(calc_hammingDist, calc_neighbor, qB, rB, qL, rL, k):
    bits = rB.shape[1]
    hamm = calc_hammingDist(torch.from_numpy(qB).float(), torch.from_numpy(rB).float())
    sim = calc_neighbor(torch.from_numpy(qL).float(), torch.from_numpy(rL).float())
    dist, ind = torch.sort(hamm, dim=1, stable=True)
    rel = sim.gather(1, ind)
    h = (2 * hamm).round().long()
    assert torch.equal(h.float() * 0.5, hamm)
    Q = qB.shape[0]
    counts = torch.zeros(Q, 2 * bits + 1, 2, dtype=torch.int64)
    for i in range(Q):
        for r in (0, 1):
            counts[i, :, r] = torch.bincount(h[i][sim[i] == r], minlength=2 * bits + 1)
    return {"idx": ind[:, :k].numpy().astype(np.int32), "dist": dist[:, :k].numpy().astype(np.float32),
            "rel": rel[:, :k].numpy().astype(np.uint8), "counts": counts.numpy().astype(np.uint32)}, hamm


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    hd, nb = reference_functions(sys.argv[1])
    rng = np.random.default_rng(20241)
    cases = {}

    def add(name, qB, rB, qL, rL, k):
        qL = qL.copy()
        qL[1] = 0                                                    # a query without a relevant item
        cases[name] = (qB, rB, qL, rL, k)

    add("b16_1000", codes(rng, 12, 16, False), codes(rng, 1000, 16, False), labels(rng, 12, 24), labels(rng, 1000, 24), 50)
    add("b64_4097", codes(rng, 10, 64, False), codes(rng, 4097, 64, False), labels(rng, 10, 24), labels(rng, 4097, 24), 100)
    add("b128_zeros_c40", codes(rng, 8, 128, True), codes(rng, 1000, 128, True), labels(rng, 8, 40), labels(rng, 1000, 40), 77)
    add("b512_qzeros", codes(rng, 4, 512, True), codes(rng, 500, 512, False), labels(rng, 4, 24), labels(rng, 500, 24), 64)
    add("b48_dbzeros", codes(rng, 6, 48, False), codes(rng, 513, 48, True), labels(rng, 6, 21), labels(rng, 513, 21), 40)
    add("b32_k1", codes(rng, 5, 32, False), codes(rng, 300, 32, False), labels(rng, 5, 8), labels(rng, 300, 8), 1)
    add("b32_kN", codes(rng, 5, 32, True), codes(rng, 300, 32, True), labels(rng, 5, 8), labels(rng, 300, 8), 300)
    one = codes(rng, 1, 64, False)
    add("b64_duplicates", np.repeat(one, 3, 0), np.repeat(one, 200, 0), labels(rng, 3, 24), labels(rng, 200, 24), 37)
    # tie groups at the k boundary, built from query 0's own histogram
    qB, rB = codes(rng, 3, 16, False), codes(rng, 1000, 16, False)
    qL, rL = labels(rng, 3, 24), labels(rng, 1000, 24)
    h0 = (2 * hd(torch.from_numpy(qB[:1]).float(), torch.from_numpy(rB).float())[0]).long()
    hist = torch.bincount(h0, minlength=33)
    cum = hist.cumsum(0)
    hstar = int((hist >= 3).nonzero()[1])                            # the second bin with a group of at least 3
    below = int(cum[hstar] - hist[hstar])
    assert below >= 1 and hist[hstar] >= 3
    add("tie_one", qB, rB, qL, rL, below + 1)
    add("tie_whole", qB, rB, qL, rL, int(cum[hstar]))

    out = {"cases": np.array(sorted(cases))}
    for name, (qB, rB, qL, rL, k) in cases.items():
        exp, hamm = expected(hd, nb, qB, rB, qL, rL, k)
        if name == "tie_one":
            assert (hamm[0] < exp["dist"][0, -1]).sum() == k - 1 and (hamm[0] == exp["dist"][0, -1]).sum() >= 3
        if name == "tie_whole":
            assert (hamm[0] <= exp["dist"][0, -1]).sum() == k and exp["dist"][0, -1] == exp["dist"][0, -2]
        if name == "b64_duplicates":
            assert (hamm == 0).all()
        assert exp["rel"][1].sum() == 0 and exp["counts"][1, :, 1].sum() == 0
        assert (exp["counts"].sum((1, 2)) == rB.shape[0]).all()
        out.update({f"{name}_qB": qB, f"{name}_rB": rB, f"{name}_qL": qL, f"{name}_rL": rL, f"{name}_k": np.int64(k)})
        out.update({f"{name}_{key}": v for key, v in exp.items()})
    assert any((out[f"{n}_dist"] % 1 == 0.5).any() for n in cases)
    path = os.path.join(HERE, "retrieval.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
