"""Times of the k-nearest search through the substring tables (SubstringTables.topk: csrc/retrieval_mih.hip cmh_mih_knn_count / _fill)
against the scan (hamming_topk's route, utils.retrieval._search on the same packed planes) in the same process, one JSON line per
measurement; medians of 5 timed regions after a warm-up, device events around each region, the two legs alternating; the results
are compared element for element before they are timed.

    python tools/mih_knn_bench.py [--shapes 15015x64,190834x128,2000000x64] [--draws random,clustered,unbalanced]
                                  [--queries 1,64,5000] [--ks 1,10,100,1000] [--max-ball M] [--centres C]

The draws are tools/mih_bench.py's: `random` (uniform codes; the queries are database codes with one bit flipped), `clustered`
(1 000 centres, every bit of an item flipped with probability 0.06; the queries are centres flipped the same way) and `unbalanced`
(uniform codes whose substring 0 takes only 256 values; at 2 000 000 x 64 only).  Per line: scan_share = the share of the queries
that SubstringTables.topk sent to the scan (radius -1, or a ball above max_ball), mean_radius = the mean r* over the queries that
stopped, mean_ball = their mean |ball(r*)|.  --centres C draws the clustered database around C centres in place of 1 000 (few
centres and a large k make balls that are a sizeable share of the database: with --max-ball N that is the measurement behind
topk's max_ball default).  Nothing is gated on these numbers."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "clip-based-cross-modal-hashing_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SHAPES = "15015x64,190834x128,2000000x64"


def measure(n, bits, draw, Qs, ks, max_ball, dev):
    import torch
    import cmh_native as N
    import mih_bench as B
    from utils import retrieval as R
    p, centres = B.planes(n, bits, draw, 1, dev)
    tables = R.SubstringTables.build(p, bits)
    g = torch.Generator(device=dev).manual_seed(2)
    for Q in Qs:
        qp = B.queries(p, centres, n, bits, Q, g, dev)
        for k in ks:
            if k > n:
                continue
            caps = R._check_topk("mih_knn_bench", bits, n, bits, k, None, max_ball, None)
            via_tables = lambda: tables._topk("mih_knn_bench", qp, k, None, None, *caps)
            via_scan = lambda: R._search("mih_knn_bench", qp, p, bits, k, None, None)
            a, b = via_tables(), via_scan()
            same = torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            radius, n_ball, _ = N.mih_knn_count(qp[0], tables.sign, bits, k, caps[0], tables.order, tables.starts)
            stopped = radius >= 0
            scanned = ~stopped | (n_ball > min(caps[1], caps[2]))
            reps = 1 if Q >= 1000 and n >= 1000000 else 3
            line = {"tool": "mih_knn_bench", "N": n, "bits": bits, "draw": draw, "centres": B.CENTRES if draw == "clustered" else None,
                    "Q": Q, "k": k, "regions": B.REGIONS,
                    "max_ball": caps[1], "outputs_equal": same, "scan_share": round(float(scanned.double().mean()), 4),
                    "mean_radius": round(float(radius[stopped].double().mean()), 2) if bool(stopped.any()) else None,
                    "mean_ball": round(float(n_ball[stopped].double().mean()), 1) if bool(stopped.any()) else None,
                    "ms": B._timed({"tables_topk": (reps, via_tables), "scan_topk": (reps, via_scan)})}
            print(json.dumps(line), flush=True)
            del a, b
    del tables
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated NxBITS")
    ap.add_argument("--draws", default="random,clustered,unbalanced")
    ap.add_argument("--queries", default="1,64,5000")
    ap.add_argument("--ks", default="1,10,100,1000")
    ap.add_argument("--max-ball", type=int, default=None, help="SubstringTables.topk's max_ball (default: its own, N // 64)")
    ap.add_argument("--centres", type=int, default=None, help="the centres of the clustered draw (default: mih_bench's 1 000)")
    args = ap.parse_args()
    if args.centres is not None:
        import mih_bench
        mih_bench.CENTRES = args.centres
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mih_knn_bench needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    Qs, ks = [int(x) for x in args.queries.split(",")], [int(x) for x in args.ks.split(",")]
    for shape in args.shapes.split(","):
        n, bits = (int(x) for x in shape.split("x"))
        for draw in args.draws.split(","):
            if draw == "unbalanced" and (n, bits) != (2000000, 64):
                continue
            measure(n, bits, draw, Qs, ks, args.max_ball, dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
