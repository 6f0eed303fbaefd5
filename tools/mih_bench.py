"""Times of multi-index hashing (csrc/retrieval_mih.hip, utils/retrieval.py::SubstringTables) on the GPU against the routes it does
not touch, one JSON line per measurement; medians of 5 timed regions after a warm-up, device events around each region, the legs
of a line alternating in one process.

    python tools/mih_bench.py [--shapes 15015x64,190834x128,2000000x64] [--legs build,lookup,unbalanced,duplicates]

build       SubstringTables.build (the nz check, m sorts of cmh_mih_build, the starts) next to BucketTable.build on the same planes.
lookup      SubstringTables lookup at r = 2, 4, 8 and the largest radius (11 / 23) for Q = 1, 64 and 5 000 queries against the scan
            (utils.retrieval._range: histogram, offsets, cmh_hamming_range) at every point and against the bucket table where r <= 2;
            the results are compared element for element before they are timed.  Two draws per shape: `random` (uniform codes; the
            queries are database codes with one bit flipped) and `clustered` (1 000 centres, every bit of an item flipped with
            probability 0.06; the queries are centres flipped the same way, so the lists are populated).  `candidates` is the mean
            number of items the kernel verifies per query: the sizes of the probed buckets, summed.
unbalanced  the same at 2 000 000 x 64 on uniform codes whose substring 0 takes only 256 values (buckets of N / 256 items there).
duplicates  CodeIndex.near_duplicates(4) against CodeIndex.duplicates(4) at 190 834 x 64, on both draws.
Nothing is gated on these numbers."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "clip-based-cross-modal-hashing_amd"))

REGIONS = 5
QUERIES = (1, 64, 5000)
SHAPES = "15015x64,190834x128,2000000x64"
CENTRES, FLIP = 1000, 0.06


def _timed(legs, regions=REGIONS):
    """legs: name -> (reps, fn), alternating, device events around each region -> name -> {median, min, max} in ms per call."""
    import torch
    for _, fn in legs.values():                                   # warm-up: code objects, workspaces, the allocator's blocks
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(regions):
        for leg, (reps, fn) in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                out = fn()
            e1.record()
            e1.synchronize()
            del out
            times[leg].append(e0.elapsed_time(e1) / reps)
    return {leg: {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)} for leg, ts in times.items()}


def _random_words(n, W, g, dev):
    import torch
    return torch.randint(-2 ** 31, 2 ** 31, (n, W), dtype=torch.int64, device=dev, generator=g).to(torch.int32)


def _flip_words(n, bits, g, dev, p=FLIP):
    """int32 [n, W]: every bit inside `bits` set with probability p, made in blocks of rows."""
    import torch
    W = (bits + 31) // 32
    weight = (torch.ones(32, dtype=torch.int64, device=dev) << torch.arange(32, device=dev))
    out = torch.empty(n, W, dtype=torch.int32, device=dev)
    for lo in range(0, n, 1 << 18):
        hi = min(n, lo + (1 << 18))
        on = torch.rand(hi - lo, W, 32, device=dev, generator=g) < p
        out[lo:hi] = ((on * weight).sum(-1) & 0xFFFFFFFF).to(torch.int32)      # (bit 31: wraps to the sign bit)
    return out


def planes(n, bits, draw, seed, dev):
    """Codes in {-1, +1} as pack_codes' planes, made on the GPU (no float copy) -> ((sign, nz) int32 [n, W], centres or None).
    random: uniform.  clustered: 1 000 uniform centres, an item = a random centre with every bit flipped with probability 0.06.
    unbalanced: uniform, but substring 0 (the low 16 bits of word 0) takes 256 values."""
    import torch
    from utils.retrieval import _nz_mask
    g = torch.Generator(device=dev).manual_seed(seed)
    W = (bits + 31) // 32
    centres = None
    if draw == "clustered":
        centres = _random_words(CENTRES, W, g, dev)
        sign = centres[torch.randint(0, CENTRES, (n,), device=dev, generator=g)] ^ _flip_words(n, bits, g, dev)
    else:
        sign = _random_words(n, W, g, dev)
        if draw == "unbalanced":
            sign[:, 0] &= ~0xFF00
    mask = _nz_mask(bits, dev)
    return ((sign & mask).contiguous(), mask.repeat(n, 1).contiguous()), centres


def queries(p, centres, n, bits, Q, g, dev):
    """Q query planes: centres flipped like the items (clustered), else database codes with one bit flipped."""
    import torch
    from utils.retrieval import _nz_mask
    mask = _nz_mask(bits, dev)
    if centres is not None:
        qs = centres[torch.randint(0, centres.shape[0], (Q,), device=dev, generator=g)] ^ _flip_words(Q, bits, g, dev)
    else:
        rows = torch.randint(0, n, (Q,), device=dev, generator=g)
        flip = torch.randint(0, bits, (Q,), device=dev, generator=g)
        qs = p[0][rows].clone()
        one = torch.ones(Q, dtype=torch.int64, device=dev)
        qs[torch.arange(Q, device=dev), flip // 32] ^= ((one << (flip % 32)) & 0xFFFFFFFF).to(torch.int32)
    return (qs & mask).contiguous(), mask.repeat(Q, 1).contiguous()


def candidates(tables, qs, radius):
    """The items the lookup verifies, per query on average: over the probed substrings, the sizes of the buckets whose key is the
    query's with at most a_j bits flipped."""
    import itertools
    import torch
    from utils.retrieval import substring_radii
    dev = qs.device
    total = torch.zeros(qs.shape[0], dtype=torch.int64, device=dev)
    for j, a in enumerate(substring_radii(tables.bits, radius)):
        if a < 0:
            continue
        s = min(16, tables.bits - 16 * j)
        flips = [0] + [sum(1 << b for b in c) for k in range(1, a + 1) for c in itertools.combinations(range(s), k)]
        key = ((qs[:, j // 2].long() >> (16 * (j % 2))) & ((1 << s) - 1))[:, None] ^ torch.tensor(flips, device=dev)[None, :]
        row = tables.starts[j].long()
        total += (row[key + 1] - row[key]).sum(1)
    return round(float(total.double().mean()), 1)


def radii_of(bits):
    top = 3 * ((bits + 15) // 16) - 1
    return [r for r in (2, 4, 8) if r < top] + [top]


def build(n, bits, dev):
    import torch
    from utils.retrieval import BucketTable, SubstringTables
    for draw in ("random", "clustered"):
        p, _ = planes(n, bits, draw, 1, dev)
        reps = 1 if n >= 1000000 else 3
        line = {"tool": "mih_bench", "leg": "build", "N": n, "bits": bits, "draw": draw, "regions": REGIONS,
                "tables": (bits + 15) // 16, "table_bytes": ((bits + 15) // 16) * (n + 65537) * 4,
                "ms": _timed({"substring_tables": (reps, lambda: SubstringTables.build(p, bits)),
                              "bucket_table": (reps, lambda: BucketTable.build(p, bits))})}
        print(json.dumps(line), flush=True)
        torch.cuda.empty_cache()


def lookup(n, bits, dev, draws=("random", "clustered"), leg="lookup"):
    import torch
    from utils import retrieval as R
    for draw in draws:
        p, centres = planes(n, bits, draw, 1, dev)
        tables = R.SubstringTables.build(p, bits)
        buckets = R.BucketTable.build(p, bits)
        g = torch.Generator(device=dev).manual_seed(2)
        for Q in QUERIES:
            qp = queries(p, centres, n, bits, Q, g, dev)
            for radius in radii_of(bits):
                via_tables = lambda: tables._lookup("mih_bench", qp, radius, None, None)
                via_scan = lambda: R._range("mih_bench", qp, p, bits, 2 * radius, None, None)
                a, b = via_tables(), via_scan()
                same = all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
                reps = 1 if Q == 5000 and n >= 1000000 else 3
                legs = {"lookup_far": (reps, via_tables), "range_search": (reps, via_scan)}
                if radius <= 2:
                    legs["lookup"] = (reps, lambda: buckets._lookup("mih_bench", qp, radius, None, None))
                line = {"tool": "mih_bench", "leg": leg, "N": n, "bits": bits, "draw": draw, "Q": Q, "radius": radius,
                        "regions": REGIONS, "hits": int(a[0][-1]), "candidates": candidates(tables, qp[0], radius),
                        "outputs_equal": same, "ms": _timed(legs)}
                print(json.dumps(line), flush=True)
                del a, b, legs
        del tables, buckets
        torch.cuda.empty_cache()


def duplicates(dev, n=190834, bits=64):
    import torch
    import cmh_native as N
    from utils.retrieval import CodeIndex
    for draw in ("random", "clustered"):
        p, _ = planes(n, bits, draw, 1, dev)
        index = CodeIndex(N.unpack_codes(p[0], p[1], bits))
        a, b = index.near_duplicates(4), index.duplicates(4)
        line = {"tool": "mih_bench", "leg": "duplicates", "N": n, "bits": bits, "draw": draw, "radius": 4, "regions": REGIONS,
                "hits": int(a[0][-1]), "outputs_equal": all(torch.equal(x, y) for x, y in zip(a, b)),
                "ms": _timed({"near_duplicates": (1, lambda: index.near_duplicates(4)), "duplicates": (1, lambda: index.duplicates(4))})}
        print(json.dumps(line), flush=True)
        del a, b, index
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated NxBITS")
    ap.add_argument("--legs", default="build,lookup,unbalanced,duplicates")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mih_bench needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    legs = args.legs.split(",")
    for shape in args.shapes.split(","):
        n, bits = (int(x) for x in shape.split("x"))
        if "build" in legs:
            build(n, bits, dev)
        if "lookup" in legs:
            lookup(n, bits, dev)
    if "unbalanced" in legs:
        lookup(2000000, 64, dev, draws=("unbalanced",), leg="unbalanced")
    if "duplicates" in legs:
        duplicates(dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
