"""Times of the bucket table (csrc/retrieval_buckets.hip, utils/retrieval.py::BucketTable) on the GPU, one JSON line per measurement;
medians of 5 timed regions after a warm-up, device events around each region, the legs of a line alternating.

    python tools/bucket_bench.py [--shapes 15015x64,190834x128,2000000x64,2000000x128] [--legs build,lookup]

build   BucketTable.build (the nz check, cmh_code_sort, cmh_code_bucket_count, the read of U, cmh_code_bucket_fill) against
        torch.unique(dim=0, return_counts=True) on the unpacked f32 codes and on the packed int32 rows.  Two draws per shape:
        `random` (every code its own bucket, every pass of the sort moves data) and `from1000` (1 000 distinct codes).
lookup  BucketTable lookup at radius 0 / 1 / 2 for Q = 1, 64 and 5 000 queries (database codes with one bit flipped) against the
        scan (utils.retrieval._range: histogram, offsets, cmh_hamming_range) at the same radius on the same planes; the two results
        are compared element for element before they are timed.
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
SHAPES = "15015x64,190834x128,2000000x64,2000000x128"


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


def planes(n, bits, draw, seed, dev):
    """Random codes in {-1, +1} as pack_codes' planes, made on the GPU (no float copy): (sign, nz) int32 [n, W]."""
    import torch
    from utils.retrieval import _nz_mask
    g = torch.Generator(device=dev).manual_seed(seed)
    W = (bits + 31) // 32
    rows = n if draw == "random" else 1000
    sign = torch.randint(-2 ** 31, 2 ** 31, (rows, W), dtype=torch.int64, device=dev, generator=g).to(torch.int32) & _nz_mask(bits, dev)
    if draw != "random":
        sign = sign[torch.randint(0, rows, (n,), device=dev, generator=g)]
    return sign.contiguous(), _nz_mask(bits, dev).repeat(n, 1).contiguous()


def build(n, bits, dev):
    import torch
    import cmh_native as N
    from utils.retrieval import BucketTable
    for draw in ("random", "from1000"):
        p = planes(n, bits, draw, 1, dev)
        table = BucketTable.build(p, bits)
        legs = {"table": (3, lambda: BucketTable.build(p, bits)),
                "unique_packed_i32": (1, lambda: torch.unique(p[0], dim=0, return_counts=True))}
        distinct = torch.unique(p[0], dim=0).shape[0]
        f32_bytes = n * bits * 4
        if f32_bytes <= 2 << 30:
            codes = N.unpack_codes(p[0], p[1], bits)
            legs["unique_f32"] = (1, lambda: torch.unique(codes, dim=0, return_counts=True))
        line = {"tool": "bucket_bench", "leg": "build", "N": n, "bits": bits, "draw": draw, "regions": REGIONS, "distinct": distinct,
                "outputs_equal": table.n_buckets == distinct, "f32_copy_bytes": f32_bytes, "plane_bytes": n * p[0].shape[1] * 4,
                "ms": _timed(legs)}
        print(json.dumps(line), flush=True)
        del legs
        torch.cuda.empty_cache()


def lookup(n, bits, dev):
    import torch
    from utils import retrieval as R
    for draw in ("random", "from1000"):
        p = planes(n, bits, draw, 1, dev)
        table = R.BucketTable.build(p, bits)
        g = torch.Generator(device=dev).manual_seed(2)
        for Q in QUERIES:
            rows = torch.randint(0, n, (Q,), device=dev, generator=g)
            flip = torch.randint(0, bits, (Q,), device=dev, generator=g)
            qs = p[0][rows].clone()
            one = torch.ones(Q, dtype=torch.int64, device=dev)
            qs[torch.arange(Q, device=dev), flip // 32] ^= ((one << (flip % 32)) & 0xFFFFFFFF).to(torch.int32)      # (bit 31: wraps to the sign bit)
            qp = (qs.contiguous(), p[1][:Q].contiguous())
            for radius in (0, 1, 2):
                via_table = lambda: table._lookup("bucket_bench", qp, radius, None, None)
                via_scan = lambda: R._range("bucket_bench", qp, p, bits, 2 * radius, None, None)
                a, b = via_table(), via_scan()
                same = all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
                reps = 1 if Q == 5000 and n >= 1000000 else 3
                line = {"tool": "bucket_bench", "leg": "lookup", "N": n, "bits": bits, "draw": draw, "Q": Q, "radius": radius,
                        "regions": REGIONS, "buckets": table.n_buckets, "hits": int(a[0][-1]), "outputs_equal": same,
                        "ms": _timed({"lookup": (reps, via_table), "hamming_range": (reps, via_scan)})}
                print(json.dumps(line), flush=True)
        del table
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated NxBITS")
    ap.add_argument("--legs", default="build,lookup")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bucket_bench needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    for shape in args.shapes.split(","):
        n, bits = (int(x) for x in shape.split("x"))
        for leg in args.legs.split(","):
            {"build": build, "lookup": lookup}[leg](n, bits, dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
