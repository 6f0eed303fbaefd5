"""cmh_code_gram (csrc/retrieval_stats.hip: the integers of the code diagnostics from the packed planes) against the only route
to the same sums before it: cmh_unpack_codes of both operands to f32 [N, K], then X.T @ Y in float64 (exact up to 2^53), and in
float32 where N < 2^24 keeps that exact.

Shapes: 15 015 x 64 bit, 190 834 x 128 bit, 2 000 000 x 64 and x 128 bit (an operand against itself: the bit correlations), and
the label case 190 834 x (21 classes against 128 bit).  Packed, resident operands; every leg warmed up; the legs alternate (native,
float64, float32) x REGIONS in one process; device events around each region of --reps calls, reported per call as median [min - max].
The float routes are timed with their unpacking and casts, which they cannot do without; `copy_bytes` is the float copy they need
(f32 rows of both operands, and the float64 casts on top for the float64 leg).  The outputs of the routes are compared on the timed
inputs: every integer equal.  ONE JSON line (also into --out).

Floors of the native call, from the shapes (printed with each shape):
  bytes   N x (2 WA + 2 WB) x 4 B once at the HBM rate (8 TB/s); the A tiles beyond the first re-read the rows from L2;
  valu    N / 64 slabs x abits x ceil(bbits / 64) lane columns x 10 wave-wide vector instructions (4 AND, 2 XOR and 4 32-bit
          popcounts, whose adds are folded in) of 4 cycles on 1024 SIMDs at 2.4 GHz: the products alone, without the transposition.
`over_floor` = the native median over the larger of the two."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "clip-based-cross-modal-hashing_amd"))

# name -> (N, abits, bbits, label case)
SHAPES = {"flickr_15015_64": (15015, 64, 64, False), "nuswide_190834_128": (190834, 128, 128, False),
          "synthetic_2000000_64": (2000000, 64, 64, False), "synthetic_2000000_128": (2000000, 128, 128, False),
          "nuswide_labels_21x128": (190834, 21, 128, True)}
REGIONS = 5


def floors_ms(n, abits, bbits):
    WA, WB = (abits + 31) // 32, (bbits + 31) // 32
    by = n * (2 * WA + 2 * WB) * 4 / 8e12
    valu = (n + 63) // 64 * abits * ((bbits + 63) // 64) * 10 * 4 / (1024 * 2.4e9)
    out = {"bytes": by * 1e3, "valu": valu * 1e3}
    out["bound"] = max(out, key=out.get)
    return out


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=",".join(SHAPES), help="comma-separated names of " + ", ".join(SHAPES))
    ap.add_argument("--reps", type=int, default=100, help="calls per timed region of the native leg (the float legs: a fifth, at least 1)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    import cmh_native as N
    if not torch.cuda.is_available():
        raise SystemExit("code_stats_bench needs a GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    result = {}
    for name in args.shapes.split(","):
        n, abits, bbits, lab = SHAPES[name]
        g = torch.Generator(device=dev).manual_seed(n + abits)
        rand = lambda bits: (torch.randint(0, 2, (n, bits), device=dev, generator=g, dtype=torch.int8) * 2 - 1).float()
        if lab:
            L = (torch.rand(n, abits, device=dev, generator=g) < 0.1).float()
            packed = N.pack_labels(L)
            a, b = (packed, packed), N.pack_codes(rand(bbits))
            del L
        else:
            a = N.pack_codes(rand(abits))
            b = a
        torch.cuda.empty_cache()

        def native():
            return N.code_gram(a, b, abits, bbits)[0]

        def floats(dt):
            X = N.unpack_codes(a[0], a[1], abits).to(dt)
            Y = X if b is a else N.unpack_codes(b[0], b[1], bbits).to(dt)
            return X.T @ Y

        legs = {"native": (native, args.reps), "float64": (lambda: floats(torch.float64), max(1, args.reps // 5))}
        if n < 2 ** 24:
            legs["float32"] = (lambda: floats(torch.float32), max(1, args.reps // 5))
        want = native()
        for leg, (fn, _) in legs.items():                          # warm-up, and the comparison on the timed inputs
            got = fn()
            if not torch.equal(got.to(torch.int64), want):
                raise SystemExit(f"{name}: {leg} differs from native")
        torch.cuda.synchronize()
        times = {leg: [] for leg in legs}
        for _ in range(REGIONS):
            for leg, (fn, reps) in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                e1.synchronize()
                times[leg].append(e0.elapsed_time(e1) / reps)
        rows = n * (abits + (0 if b is a else bbits))
        line = {"N": n, "abits": abits, "bbits": bbits, "floors_ms": floors_ms(n, abits, bbits),
                "packed_bytes": sum(t.numel() * 4 for t in set(a + b)),
                "workspace_bytes": N.lib().cmh_code_gram_workspace_bytes(n, abits, bbits, 0),
                "copy_bytes": {"float32": rows * 4, "float64": rows * 12}}
        line.update({leg: spread(ms) for leg, ms in times.items()})
        fl = line["floors_ms"]
        line["over_floor"] = line["native"]["median_ms"] / fl[fl["bound"]]
        for leg in ("float64", "float32"):
            if leg in line:
                line[f"{leg}_over_native"] = line[leg]["median_ms"] / line["native"]["median_ms"]
        result[name] = line
        show = lambda s: f"{s['median_ms']:.4f} [{s['min_ms']:.4f} - {s['max_ms']:.4f}] ms"
        print(f"# {name}: native {show(line['native'])}, float64 {show(line['float64'])}"
              + (f", float32 {show(line['float32'])}" if "float32" in line else "")
              + f"; floors bytes {fl['bytes']:.4f} valu {fl['valu']:.4f} ms, over floor {line['over_floor']:.2f}x; float copy "
              + f"{line['copy_bytes']['float64'] / 1e6:.1f} MB (f64 route), packed {line['packed_bytes'] / 1e6:.1f} MB", flush=True)
        del a, b, want, got
        torch.cuda.empty_cache()
    text = json.dumps(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
