"""Top-k search and distance histograms (csrc/retrieval.hip) against the only route to the same neighbours without them:
hamming_map(tie_order=TIE_STABLE, want_perm=True)[2][:, :k], a full sort of N per query and a [Q, N] int32 ranking.

Shapes: 5000 x 15 015 x 64 bit (bench.py's default --map-db) and 5000 x 190 834 x 128 bit (NUS-WIDE).  Packed, resident operands;
every leg warmed up; legs alternate (ranking, topk k=100, topk k=1000, histogram, graded topk k=100, graded topk k=1000, label
histogram) x REGIONS in one process; device events around each region; a region of the new legs is several calls (a single one is
too short to time) and is reported per call.  The outputs of the two routes are compared on the timed inputs, and the graded
search's idx / dist with the plain search's.  One JSON line per shape (also into --out).

The graded legs (hamming_topk_graded, label_overlap_hist) are reported against the plain legs of the same run: `graded_over_plain`
= median over median at the same k, `labelhist_over_hist` = the label histogram over the distance histogram.

Floors of one pass over the database, from the shapes (printed with the line):
  bytes     query tiles x N x (2 W + LW) x 4 B: the database is re-read once per tile of 64 queries, from L2 (34.5 TB/s aggregate);
  increments  query tiles x N wave-wide LDS increments, one per 4 LDS cycles per CU (the cost of a 32-bit LDS write instruction),
            256 CUs at 2.4 GHz;
  valu      query tiles x N x (5 W + 8) wave-wide vector instructions of 4 cycles on 1024 SIMDs at 2.4 GHz (and / xor / and / two
            popcounts and their sums per word, the distance, the relevance test, the address).
The search makes two passes (the second without increments for most items).

--sharded runs the sharded leg instead (utils/retrieval.py: shards of the database searched one by one, the lists folded by
cmh_topk_merge), synthetic codes, same rules (device events, REGIONS regions of --reps calls, median [min - max], legs alternating):
  (a) 5000 x 190 834 x 128 bit, k = 100 and 1000, as 1 / 2 / 4 shards.  One shard is the single native call (the baseline: the
      search as it was before sharding existed); `over_one_shard` = median over median is the price of sharding plus merging.
      The lists of 2 and 4 shards are compared with the one-shard list on the timed inputs.
  (b) 5000 x 2 000 000 x 64 bit, k = 1000, at the default shard size (4 shards): no baseline, one call refuses it.  64 rows are
      compared with torch.sort(stable=True) of the full distance rows.  Reported with the floor of two passes over the same
      item count.
`merge` is a leg of its own: the fold of the per-shard lists alone (the merge launches of one search on lists computed before
the timed regions), and `merge_share` its median over the search's.

--map runs the mAP legs instead: the mAP by counting (hamming_ap_partial + ap_finish: no ranking) against the two routes there were,
hamming_map(TIE_STABLE) (the same tie order: a radix sort of N keys per query) and hamming_map(TIE_REFERENCE), at the two shapes
above, same rules.  `hist` (the counting route's first pass alone) runs next to them.  Per-query APs of the counting route are
compared with the stable ranking's on the timed inputs (2e-6).  Then 5000 x 2 000 000 x 64 bit in four shards
(utils.retrieval._map_count), which no other route takes: 16 of its APs are compared with a float64 AP on torch.sort(stable=True).

--range runs the radius-search legs instead: utils.retrieval._range (histogram -> offsets -> T read back -> cmh_hamming_range) against
the only route to the same lists without it, hamming_topk(k = the largest ball of any query, read off the histogram) and a trim of
every row, at the two shapes above and, per shape, the two radii at which the mean ball is nearest 100 and 1000 items (read off the
histogram).  Same rules (warm-up, legs alternating in one process, device events around regions of --reps calls); `fill` (the
native call alone on offsets made before the timed regions) and `hist` run next to them.  The lists of the two routes are compared
on the timed inputs.  Reported per radius: both times, the output bytes of both routes (T x 9 against Q x kmax x 9), and the floors
of the new route's three passes over the database (hist, and hist + fill inside the native call) plus its output bytes over HBM
bandwidth (8 TB/s).  ONE JSON line for all shapes.

--rank runs the target-rank legs instead: the ranks of paired items by counting (utils.retrieval._target_counts: the gather of the
targets' planes and ONE cmh_hamming_rank; `native` is the call alone on planes gathered before the timed regions) against the only
route there was, hamming_topk(k = N) and a search of the [Q, N] index matrix for the target (`topk_lookup`), at 5000 x 5000 x 64 bit
(identity pairing) and 5000 x 190 834 x 128 bit (one random target per query).  Same rules (warm-up, legs alternating in one
process, device events around regions of --reps calls; the baseline runs once per region); both routes' positions are compared on
the timed inputs.  A baseline that cannot be allocated is recorded as such.  Then 5000 x 2 000 000 x 64 bit in four shards, which no
other route takes: 16 of its rows are compared with counts made from the full distance rows.  One JSON line per shape.

--few runs the few-query legs instead: ONE cmh_hamming_topk_few over the whole database (csrc/retrieval_few.hip: lanes own items)
against the route such a search took before it existed, the tiles kernels (lanes own queries) as utils.retrieval._search runs them
at the default shard size: one cmh_hamming_topk at 190 834 x 128 bit, four shards and three merges at 2 000 000 x 64 bit.
Q = 1, 2, 4, 8, 16, 32, 64 and k = 10, 1000 on both databases; a query is a database item with a tenth of its bits flipped.  Same
rules (warm-up, legs alternating in one process, device events around regions of --reps calls, median [min - max], packed resident
operands); both routes' lists are compared on the timed inputs.  `queries_few` is the largest Q of that list at which the new
call's maximum lies below the tiles route's minimum on both databases at k = 1000 (utils.retrieval.QUERIES_FEW is set from it);
`bar_q1` says whether the ranges are apart at Q = 1 on both databases at both k.  Floor per shape: two passes over N x 2 W x 4 bytes
at the HBM rate (8 TB/s) plus Q x N / 64 wave-wide item groups x (5 W + 8) vector instructions of 4 cycles on 1024 SIMDs at 2.4 GHz
per pass.  Then, without a bar, the wall time of one interactive query against the 2 000 000-item index: caption -> tokens -> codes
(query.py::QueryEncoder on a ViT-B/32-sized DSPH model with random weights) -> 10 neighbours, warm, median of 20, split into
tokenise / encode / search (host clock around a device synchronise).  ONE JSON line.

--soft runs the soft-query legs instead: cmh_soft_topk (csrc/retrieval_soft.hip: the weighted distance of a real-valued query, 30 bits
+ 1 bins) against cmh_hamming_topk_few (2 bits + 1 bins) on the same database planes in the same process, at Q = 1, 64 and k = 10,
1000 on both databases of --few; a soft query is tanh of a normal draw scaled towards a database item, the Hamming query its sign.
Same rules (warm-up, legs alternating, device events around regions of --reps calls, median [min - max], packed resident operands;
`soft_planes` times the quantiser with its flag read back).  Where soft and Hamming must agree (all |w| = 15) the lists are compared on the timed
database.  Reported per (shape, Q, k): both times and soft / few, and both workspaces.  CMH_SOFT_GROUP=g in the environment
pins g queries per workgroup, CMH_SOFT_MIN_CHUNK=c the fewest items of a chunk, in place of the plan's choices, for an A/B of the
same line.  ONE JSON line.

--soft-map runs the soft-mAP legs instead: utils.retrieval's soft mAP by counting over the whole database (cmh_soft_ap, blocks of 64
queries; csrc/retrieval_soft.hip) at the two shapes of --shapes, alternating with `binary`, mean_average_precision's counting route
(cmh_hamming_ap_partial + cmh_ap_finish, kernels of csrc/retrieval.hip) on the SIGN codes of the same queries.  A soft query is
tanh of the label projection plus noise, the database the sign of the same model.  Same rules (warm-up, legs alternating, device
events around regions of one call, median [min - max], packed resident operands; the quantiser is inside the soft leg).  The first
16 queries' AP, R and rank sum are compared with a float64 stable sort on the timed inputs.  Reported per shape: both times, soft /
binary, both mAPs and the mean AUC.  The stages of one call (relevance words, histogram pass, totals, prefixes, bases, rank pass,
finish) are separate kernels: a kernel trace of this leg gives the time of each.  One JSON line per shape.

--masked runs the filtered-search legs instead: cmh_hamming_topk_few_masked (the allow-mask in the walk: one 64-bit word per 64
items) on both databases of --few at Q = 1, 64 and k = 10, 1000 under random masks that admit a share 1.0 / 0.5 / 0.1 / 0.01 of the
items, against (b) `few`, the unmasked cmh_hamming_topk_few on the same operands (at share 1.0 the difference is the price of the
filter), (c) `gather`, the only route there was: the admitted rows gathered into a second packed database (mask -> booleans ->
nonzero, which reads the count back; two row gathers), the unmasked search of that with k' = min(k, admitted), and the indices
mapped back, with its allocations; and `gather_cached`, (c) on a subset gathered BEFORE the timed regions: what (c) costs while the
filter does not change.  Same rules (warm-up, legs alternating, device events around regions of --reps calls, median [min - max],
packed resident operands); the lists of (a) and (c) are compared on the timed inputs.  ONE JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "clip-based-cross-modal-hashing_amd"))

SHAPES = {"flickr_15015_64": (5000, 15015, 64, 24), "nuswide_190834_128": (5000, 190834, 128, 21)}
REGIONS = 5


def floors_ms(Q, n, bits, classes, passes):
    tiles, W, LW = (Q + 63) // 64, (bits + 31) // 32, (classes + 31) // 32
    by = tiles * n * (2 * W + LW) * 4 / 34.5e12
    inc = tiles * n * 4 / (256 * 2.4e9)
    valu = tiles * n * (5 * W + 8) * 4 / (1024 * 2.4e9)
    out = {"bytes": by * 1e3 * passes, "increments": inc * 1e3, "valu": valu * 1e3 * passes}
    out["bound"] = max(out, key=out.get)
    return out


SHARDED = {"nuswide_190834_128": (5000, 190834, 128, 21, (100, 1000), (1, 2, 4)),
           "synthetic_2000000_64": (5000, 2000000, 64, 24, (1000,), (None,))}


def sharded(args):
    import torch
    import cmh_native as N
    import utils.retrieval as R
    dev = torch.device("cuda:0")
    for name, (Q, n, K, C, ks, cuts) in SHARDED.items():
        g = torch.Generator(device=dev).manual_seed(1)
        rL = (torch.rand(n, C, generator=g, device=dev) < 0.1).float()
        qL = (torch.rand(Q, C, generator=g, device=dev) < 0.1).float()
        rL[:, 0] = 1.0
        qL[:, 0] = 1.0
        Wm = torch.randn(C, K, generator=g, device=dev)
        mk = lambda lab: torch.sign(lab @ Wm + 0.5 * torch.randn(lab.shape[0], K, generator=g, device=dev) + 1e-3)
        rB, qB = mk(rL), mk(qL)
        rp, qp = N.pack_codes(rB), N.pack_codes(qB)
        rl, ql = N.pack_labels(rL), N.pack_labels(qL)
        step = lambda c: N.TOPK_MAX if c is None else (n + c - 1) // c
        legs, lists = {}, {}
        for k in ks:
            for c in cuts:
                items = step(c)
                shards = R._cuts(n, items)
                tag = f"k{k}_s{len(shards)}"
                legs[tag] = (lambda k=k, items=items: R._search("bench", qp, rp, K, k, ql, rl, items))
                if len(shards) > 1:
                    # the per-shard lists of one search, computed once: the merge leg folds them as _search does
                    per = [N.hamming_topk(qp, R._rows(rp, sc, n), K, min(k, sc[1] - sc[0]), ql, R._rows(rl, sc, n)) for sc in shards]
                    lists[tag] = (k, shards, per)

                    def fold(tag=tag):
                        k, shards, per = lists[tag]
                        run, flat = per[0], [None, None]
                        for s, (sc, b) in enumerate(zip(shards[1:], per[1:])):
                            run = R._fold(run, b, sc, k, flat, s)
                        return run
                    legs["merge_" + tag] = fold
        outs = {tag: fn() for tag, fn in legs.items()}                    # warm-up, and the outputs on the timed inputs
        same = True
        for tag, out in outs.items():
            if tag.startswith("merge_"):
                same = same and all(bool(torch.equal(a, b)) for a, b in zip(out, outs[tag[6:]][:3]))
            elif f"{tag.split('_')[0]}_s1" in outs:
                same = same and all(bool(torch.equal(a, b)) for a, b in zip(out[:3], outs[f"{tag.split('_')[0]}_s1"][:3]))
            else:                                                         # no one-shard list: 64 rows against the full stable sort
                full = 0.5 * (K - qB[:64] @ rB.T)
                d, i = torch.sort(full, dim=1, stable=True)
                k = out[0].shape[1]
                same = same and bool(torch.equal(out[0][:64].long(), i[:, :k])) and bool(torch.equal(out[1][:64], d[:, :k]))
                del full, d, i
        del outs
        torch.cuda.synchronize()
        times = {tag: [] for tag in legs}
        for _ in range(REGIONS):
            for tag, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    out = fn()
                e1.record()
                e1.synchronize()
                del out
                times[tag].append(e0.elapsed_time(e1) / args.reps)
        line = {"tool": "retrieval_bench", "leg": "sharded", "shape": name, "Q": Q, "N": n, "bits": K, "classes": C, "regions": REGIONS,
                "outputs_equal": same, "ms": {}}
        for tag, ts in times.items():
            line["ms"][tag] = {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}
        for tag in times:
            if tag.startswith("merge_"):
                line["ms"][tag[6:]]["merge_share"] = round(line["ms"][tag]["median"] / line["ms"][tag[6:]]["median"], 4)
            else:
                one = f"{tag.split('_')[0]}_s1"
                if one in times:
                    line["ms"][tag]["over_one_shard"] = round(line["ms"][tag]["median"] / line["ms"][one]["median"], 4)
                else:
                    fl = floors_ms(Q, n, K, C, 2)
                    line["ms"][tag]["floor_ms"] = {k: (round(v, 4) if k != "bound" else v) for k, v in fl.items()}
                    line["ms"][tag]["share_of_floor"] = round(fl[fl["bound"]] / line["ms"][tag]["median"], 4)
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(text + "\n")
        if not same:
            raise SystemExit(f"{name}: the sharded search disagrees with the search of the whole database")
        del rB, qB, rp, qp, rl, ql, rL, qL, legs, lists


def _timed(legs, regions):
    """legs: name -> (reps, fn), alternating, device events around each region -> name -> {median, min, max} in ms per call."""
    import torch
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


def _emit(args, line):
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")


def map_legs(args):
    import torch
    import cmh_native as N
    import utils.retrieval as R
    dev = torch.device("cuda:0")

    def operands(Q, n, K, C):
        g = torch.Generator(device=dev).manual_seed(1)
        rL = (torch.rand(n, C, generator=g, device=dev) < 0.1).float()
        qL = (torch.rand(Q, C, generator=g, device=dev) < 0.1).float()
        rL[:, 0] = 1.0                                            # every query has relevant items: the ranking skips none
        qL[:, 0] = 1.0
        qL[:, 0][::7] = 0.0                                       # ... but not every pair is relevant
        rL[:, 0][::3] = 0.0
        Wm = torch.randn(C, K, generator=g, device=dev)
        mk = lambda lab: torch.sign(lab @ Wm + 0.5 * torch.randn(lab.shape[0], K, generator=g, device=dev) + 1e-3)
        return mk(qL), mk(rL), qL, rL

    for name in args.shapes:
        Q, n, K, C = SHAPES[name]
        qB, rB, qL, rL = operands(Q, n, K, C)
        qp, rp, ql, rl = N.pack_codes(qB), N.pack_codes(rB), N.pack_labels(qL), N.pack_labels(rL)
        del qB, rB

        def counting():
            s, counts = N.hamming_ap_partial(qp, rp, K, ql, rl, want_counts=True)
            return N.ap_finish(s, counts, K)

        legs = {
            "counting": (args.reps, counting),
            "hist": (args.reps, lambda: N.hamming_hist(qp, rp, K, ql, rl)),
            "stable": (1, lambda: N.hamming_map(qp, ql, rp, rl, K, C, tie_order=N.TIE_STABLE)[:2]),
            "reference": (1, lambda: N.hamming_map(qp, ql, rp, rl, K, C, tie_order=N.TIE_REFERENCE)[:2]),
        }
        outs = {leg: fn() for leg, (_, fn) in legs.items()}        # warm-up, and the outputs on the timed inputs
        d_ap = float((outs["counting"][1].double() - outs["stable"][1].double()).abs().max())
        d_map = abs(float(outs["counting"][0]) - float(outs["stable"][0]))
        relevant_share = float(outs["hist"][:, :, 1].sum().double() / (Q * n))
        del outs
        torch.cuda.synchronize()
        line = {"tool": "retrieval_bench", "leg": "map", "shape": name, "Q": Q, "N": n, "bits": K, "classes": C, "regions": REGIONS,
                "relevant_share": round(relevant_share, 4), "max_ap_diff_vs_stable": d_ap, "map_diff_vs_stable": d_map,
                "outputs_equal": d_ap <= 2e-6 and d_map <= 2e-6, "ms": _timed(legs, REGIONS)}
        for base in ("stable", "reference"):
            line["ms"]["counting"][f"{base}_over_counting"] = round(line["ms"][base]["median"] / line["ms"]["counting"]["median"], 3)
        line["ms"]["counting"]["over_hist"] = round(line["ms"]["counting"]["median"] / line["ms"]["hist"]["median"], 3)
        _emit(args, line)
        if not line["outputs_equal"]:
            raise SystemExit(f"{name}: the mAP by counting disagrees with the stable ranking")
        del qp, rp, ql, rl, legs
    if args.no_large:
        return
    Q, n, K, C = 5000, 2000000, 64, 24
    qB, rB, qL, rL = operands(Q, n, K, C)
    qp, rp, ql, rl = N.pack_codes(qB), N.pack_codes(rB), N.pack_labels(qL), N.pack_labels(rL)
    legs = {"counting": (1, lambda: R._map_count("bench", qp, rp, K, ql, rl)),
            "search_k1000": (1, lambda: R._search("bench", qp, rp, K, 1000, ql, rl)[:3])}
    mp, ap = legs["counting"][1]()
    legs["search_k1000"][1]()
    rows = 16
    order = torch.sort((K - qB[:rows] @ rB.T), dim=1, stable=True)[1]
    hits = ((qL[:rows] @ rL.T) > 0).gather(1, order)
    del order
    pos = torch.arange(1, n + 1, device=dev, dtype=torch.float64)
    want = ((hits.cumsum(1).double() / pos) * hits).sum(1) / hits.sum(1).clamp(min=1)
    d_ap = float((ap[:rows].double() - want).abs().max())
    del hits, pos, qB, rB
    torch.cuda.synchronize()
    line = {"tool": "retrieval_bench", "leg": "map", "shape": "synthetic_2000000_64", "Q": Q, "N": n, "bits": K, "classes": C,
            "shards": len(R._cuts(n, R.SHARD_ITEMS)), "regions": REGIONS, "map": float(mp), "max_ap_diff_vs_float64_sort": d_ap,
            "outputs_equal": d_ap <= 2.4e-7, "ms": _timed(legs, REGIONS)}
    line["ms"]["counting"]["over_search_k1000"] = round(line["ms"]["counting"]["median"] / line["ms"]["search_k1000"]["median"], 3)
    _emit(args, line)
    if not line["outputs_equal"]:
        raise SystemExit("synthetic_2000000_64: the sharded mAP by counting disagrees with the float64 AP on a stable sort")


def range_legs(args):
    import torch
    import cmh_native as N
    import utils.retrieval as R
    dev = torch.device("cuda:0")
    line = {"tool": "retrieval_bench", "leg": "range", "regions": REGIONS, "reps": args.reps, "outputs_equal": True, "shapes": {}}
    for name in args.shapes:
        Q, n, K, C = SHAPES[name]
        g = torch.Generator(device=dev).manual_seed(1)
        rL = (torch.rand(n, C, generator=g, device=dev) < 0.1).float()
        qL = (torch.rand(Q, C, generator=g, device=dev) < 0.1).float()
        rL[:, 0] = 1.0
        qL[:, 0] = 1.0
        Wm = torch.randn(C, K, generator=g, device=dev)
        mk = lambda lab: torch.sign(lab @ Wm + 0.5 * torch.randn(lab.shape[0], K, generator=g, device=dev) + 1e-3)
        qp, rp, ql, rl = N.pack_codes(mk(qL)), N.pack_codes(mk(rL)), N.pack_labels(qL), N.pack_labels(rL)
        balls = N.hamming_hist(qp, rp, K, ql, rl).sum(2).cumsum(1)          # [Q, 2K+1]: ball sizes by half-radius
        mean = balls.double().mean(0).cpu()
        shape = {"Q": Q, "N": n, "bits": K, "classes": C, "radii": {}}
        for target in (100, 1000):
            hr = int((mean.clamp(min=1e-9).log() - torch.log(torch.tensor(float(target), dtype=torch.float64))).abs().argmin())
            off = torch.zeros(Q + 1, dtype=torch.int64, device=dev)
            off[1:] = balls[:, hr].cumsum(0)
            T, kmax = int(off[-1]), int(balls[:, hr].max())
            row_off = off[:-1].contiguous()
            bufs = (torch.empty(T, dtype=torch.int32, device=dev), torch.empty(T, dtype=torch.float32, device=dev),
                    torch.empty(T, dtype=torch.uint8, device=dev))

            def trim():
                ball = N.hamming_hist(qp, rp, K, ql, rl)[:, :hr + 1].sum((1, 2))
                k = int(ball.max())
                rows = N.hamming_topk(qp, rp, K, k, ql, rl)
                head = torch.arange(k, device=dev)[None, :] < ball[:, None]
                return tuple(r[head] for r in rows)

            big = Q * kmax > 5e7                                              # the baseline's Q x kmax outputs: one call per region then
            legs = {"range": (args.reps, lambda: R._range("bench", qp, rp, K, hr, ql, rl)),
                    "topk_trim": (1 if big else args.reps, trim),
                    "fill": (args.reps, lambda: N.hamming_range(qp, rp, K, hr, ql, rl, row_off=row_off, out=bufs)),
                    "hist": (args.reps, lambda: N.hamming_hist(qp, rp, K, ql, rl))}
            new, old = legs["range"][1](), legs["topk_trim"][1]()           # warm-up, and the outputs on the timed inputs
            legs["fill"][1](), legs["hist"][1]()
            same = bool(torch.equal(new[0], off)) and all(bool(torch.equal(a, b)) for a, b in zip(new[1:], old))
            same = same and all(bool(torch.equal(a, b)) for a, b in zip(new[1:], bufs))
            del new, old
            torch.cuda.synchronize()
            ms = _timed(legs, REGIONS)
            fl = floors_ms(Q, n, K, C, 3)
            fl["out_bytes"] = T * 9 / 8e12 * 1e3
            ms["range"]["floor_ms"] = {k: (round(v, 4) if k != "bound" else v) for k, v in fl.items()}
            ms["range"]["over_topk_trim"] = round(ms["range"]["median"] / ms["topk_trim"]["median"], 4)
            ms["range"]["over_hist_plus_fill"] = round(ms["range"]["median"] / (ms["hist"]["median"] + ms["fill"]["median"]), 4)
            shape["radii"][f"mean_ball_{target}"] = {
                "radius": hr / 2, "radius_h": hr, "mean_ball": round(float(mean[hr]), 2), "largest_ball": kmax, "T": T,
                "out_bytes_range": T * 9, "out_bytes_topk_trim": Q * kmax * 9, "outputs_equal": same, "ms": ms}
            line["outputs_equal"] = line["outputs_equal"] and same
            del bufs, legs
        line["shapes"][name] = shape
        del qp, rp, ql, rl, balls
    _emit(args, line)
    if not line["outputs_equal"]:
        raise SystemExit("the radius search disagrees with hamming_topk(k = largest ball) cut at the balls")


RANK = {"paired_5000_64": (5000, 5000, 64, True), "nuswide_190834_128": (5000, 190834, 128, False)}


def rank_legs(args):
    import torch
    import cmh_native as N
    import utils.retrieval as R
    dev = torch.device("cuda:0")

    def operands(Q, n, K, identity):
        g = torch.Generator(device=dev).manual_seed(1)
        rB = torch.sign(torch.randn(n, K, generator=g, device=dev) + 1e-3)
        t = torch.arange(Q, device=dev) if identity else torch.randint(0, n, (Q,), generator=g, device=dev)
        flip = torch.rand(Q, K, generator=g, device=dev) < 0.1                     # a query = its item with a tenth of the bits flipped
        return torch.where(flip, -rB[t], rB[t]), rB, t

    def row_counts(qB, rB, t, rows):
        h = (qB.shape[1] - qB[:rows] @ rB.T).long()
        ht = h.gather(1, t[:rows, None])
        before = (h == ht) & (torch.arange(rB.shape[0], device=dev)[None, :] < t[:rows, None])
        return torch.stack([(h < ht).sum(1), before.sum(1), (h == ht).sum(1)], 1)

    for name, (Q, n, K, identity) in RANK.items():
        qB, rB, t = operands(Q, n, K, identity)
        qp, rp = N.pack_codes(qB), N.pack_codes(rB)
        tp = tuple(x.index_select(0, t) for x in rp)
        bound = t.to(torch.int32)[:, None].contiguous()

        def lookup():
            idx = N.hamming_topk(qp, rp, K, n)[0]
            return (idx == t[:, None]).to(torch.uint8).argmax(1)

        legs = {"counting": (args.reps, lambda: R._target_counts("bench", qp, rp, K, t)),
                "native": (args.reps, lambda: N.hamming_rank(qp, rp, K, tp, bound))}
        counts = legs["counting"][1]()                                            # warm-up, and the outputs on the timed inputs
        same = bool(torch.equal(counts, legs["native"][1]().long())) and bool(torch.equal(counts[:64, 0], row_counts(qB, rB, t, 64)))
        line = {"tool": "retrieval_bench", "leg": "rank", "shape": name, "Q": Q, "N": n, "bits": K, "pairing": "identity" if identity else "random",
                "regions": REGIONS, "reps": args.reps, "mean_ties": round(float(counts[:, 0, 2].double().mean()), 2)}
        try:
            pos = lookup()
            same = same and bool(torch.equal(pos, counts[:, 0, 0] + counts[:, 0, 1]))
            del pos
            legs["topk_lookup"] = (1, lookup)
            line["topk_lookup_bytes"] = Q * n * 8
        except torch.cuda.OutOfMemoryError:
            line["topk_lookup"] = f"cannot allocate the [Q, N] lists of k = N ({Q * n * 8} bytes)"
        torch.cuda.synchronize()
        line.update(outputs_equal=same, ms=_timed(legs, REGIONS))
        fl = {k: v for k, v in floors_ms(Q, n, K, 0, 1).items() if k in ("bytes", "valu")}      # (no columns: no LDS increments)
        line["ms"]["native"]["floor_ms"] = dict({k: round(v, 4) for k, v in fl.items()}, bound=max(fl, key=fl.get))
        if "topk_lookup" in legs:
            line["ms"]["counting"]["over_topk_lookup"] = round(line["ms"]["counting"]["median"] / line["ms"]["topk_lookup"]["median"], 4)
        _emit(args, line)
        if not same:
            raise SystemExit(f"{name}: the ranks by counting disagree with the target's column in hamming_topk(k = N)")
        del qB, rB, t, qp, rp, tp, bound, legs, counts
    if args.no_large:
        return
    Q, n, K = 5000, 2000000, 64
    qB, rB, t = operands(Q, n, K, False)
    qp, rp = N.pack_codes(qB), N.pack_codes(rB)
    legs = {"counting": (1, lambda: R._target_counts("bench", qp, rp, K, t))}
    counts = legs["counting"][1]()
    same = bool(torch.equal(counts[:16, 0], row_counts(qB, rB, t, 16)))
    torch.cuda.synchronize()
    line = {"tool": "retrieval_bench", "leg": "rank", "shape": "synthetic_2000000_64", "Q": Q, "N": n, "bits": K, "pairing": "random",
            "shards": len(R._cuts(n, R.SHARD_ITEMS)), "regions": REGIONS, "outputs_equal": same, "topk_lookup": "no such route: k <= 524 287",
            "ms": _timed(legs, REGIONS)}
    _emit(args, line)
    if not same:
        raise SystemExit("synthetic_2000000_64: the sharded ranks by counting disagree with counts made from the distance rows")


FEW = {"nuswide_190834_128": (190834, 128), "synthetic_2000000_64": (2000000, 64)}
FEW_QS = (1, 2, 4, 8, 16, 32, 64)
FEW_KS = (10, 1000)


def few_floor_ms(Q, n, bits):
    W = (bits + 31) // 32
    by = 2 * n * 2 * W * 4 / 8e12
    valu = 2 * (Q * n / 64) * (5 * W + 8) * 4 / (1024 * 2.4e9)
    return {"bytes": round(by * 1e3, 5), "valu": round(valu * 1e3, 5), "sum": round((by + valu) * 1e3, 5)}


def few_legs(args):
    import tempfile
    import time
    import torch
    import cmh_native as N
    import utils.retrieval as R
    dev = torch.device("cuda:0")
    line = {"tool": "retrieval_bench", "leg": "few", "regions": REGIONS, "reps": args.reps, "outputs_equal": True, "shapes": {}}
    apart = {}                                                     # (shape, Q, k) -> the new call's max < the tiles route's min
    for name, (n, K) in FEW.items():
        g = torch.Generator(device=dev).manual_seed(1)
        rB = torch.sign(torch.randn(n, K, generator=g, device=dev) + 1e-3)
        t = torch.randint(0, n, (max(FEW_QS),), generator=g, device=dev)
        flip = torch.rand(max(FEW_QS), K, generator=g, device=dev) < 0.1
        qp_all, rp = N.pack_codes(torch.where(flip, -rB[t], rB[t])), N.pack_codes(rB)
        del rB, flip
        shape = {"N": n, "bits": K, "shards_of_the_tiles_route": len(R._cuts(n, R.SHARD_ITEMS)), "ms": {}}
        for Q in FEW_QS:
            qp = tuple(x[:Q].contiguous() for x in qp_all)
            legs = {}
            for k in FEW_KS:
                legs[f"few_k{k}"] = (args.reps, lambda k=k: N.hamming_topk_few(qp, rp, K, k))
                legs[f"tiles_k{k}"] = (args.reps, lambda k=k: R._search("bench", qp, rp, K, k, None, None, shard_items=R.SHARD_ITEMS)[:2])
            outs = {leg: fn() for leg, (_, fn) in legs.items()}    # warm-up, and the outputs of both routes on the timed inputs
            same = all(bool(torch.equal(a, b)) for k in FEW_KS for a, b in zip(outs[f"few_k{k}"], outs[f"tiles_k{k}"]))
            line["outputs_equal"] = line["outputs_equal"] and same
            del outs
            torch.cuda.synchronize()
            ms = _timed(legs, REGIONS)
            for k in FEW_KS:
                apart[(name, Q, k)] = ms[f"few_k{k}"]["max"] < ms[f"tiles_k{k}"]["min"]
                ms[f"few_k{k}"]["tiles_over_few"] = round(ms[f"tiles_k{k}"]["median"] / ms[f"few_k{k}"]["median"], 2)
                ms[f"few_k{k}"]["apart"] = apart[(name, Q, k)]
            ms["floor_ms"] = few_floor_ms(Q, n, K)
            ms["outputs_equal"] = same
            shape["ms"][f"Q{Q}"] = ms
        line["shapes"][name] = shape
        if name != "synthetic_2000000_64":
            del qp_all, rp
    holds = [Q for Q in FEW_QS if all(apart[(name, Q, 1000)] for name in FEW)]
    line["queries_few"] = max(holds) if holds else 0
    line["queries_few_holds_at"] = holds
    line["bar_q1"] = all(apart[(name, 1, k)] for name in FEW for k in FEW_KS)
    line["queries_few_committed"] = R.QUERIES_FEW

    # one interactive query against the 2 000 000-item index (rp, of the last shape): caption -> tokens -> codes -> 10 neighbours
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import recipe
    from model.DSPH import MDSPH
    from query import QueryEncoder
    n, K = FEW["synthetic_2000000_64"]
    sd = {k: torch.from_numpy(v) for k, v in recipe.clip_state_dict(recipe.CLIP_VITB32, 7).items()}
    state = MDSPH(outputDim=K, clipPath=sd, saveDir=tempfile.mkdtemp(prefix="cmh_few_")).state_dict()
    enc = QueryEncoder("DSPH", state, sd, K, bpe_path=os.path.join(ROOT, "tests", "golden", "clip_bpe_merges_48894.txt.gz"))
    caption = ["a dog on a beach"]
    parts = {"tokenise": [], "encode": [], "search": [], "total": []}
    for i in range(5 + 20):                                        # five warm-up rounds, then the 20 that count
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tokens = enc.tokenize(caption)
        t1 = time.perf_counter()
        codes = enc.encode_tokens(tokens)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        idx, dist, _, _ = R._search("bench", R._codes(codes, dev), rp, K, 10, None, None)      # (CodeIndex.search on resident planes)
        first = idx[0].tolist()                                    # (the answer on the host: what retrieve.py prints)
        t3 = time.perf_counter()
        if i >= 5:
            for key, v in (("tokenise", t1 - t0), ("encode", t2 - t1), ("search", t3 - t2), ("total", t3 - t0)):
                parts[key].append(v * 1e3)
    line["one_query_ms"] = {key: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                            for key, v in parts.items()}
    line["one_query_ms"]["model"] = "DSPH on ViT-B/32 (random weights), f32 GEMMs, 64 bit; index 2 000 000 x 64 bit; k = 10"
    line["one_query_ms"]["neighbours"] = len(first)
    _emit(args, line)
    if not line["outputs_equal"]:
        raise SystemExit("the few-query search disagrees with the tiles route")


SOFT_QS = (1, 64)


def soft_legs(args):
    import torch
    import cmh_native as N
    dev = torch.device("cuda:0")
    line = {"tool": "retrieval_bench", "leg": "soft", "regions": REGIONS, "reps": args.reps, "agree_where_they_must": True,
            "soft_group_pinned": os.environ.get("CMH_SOFT_GROUP", ""), "soft_min_chunk_pinned": os.environ.get("CMH_SOFT_MIN_CHUNK", ""),
            "shapes": {}}
    for name, (n, K) in FEW.items():
        g = torch.Generator(device=dev).manual_seed(1)
        rB = torch.sign(torch.randn(n, K, generator=g, device=dev) + 1e-3)
        t = torch.randint(0, n, (max(SOFT_QS),), generator=g, device=dev)
        u_all = torch.tanh(torch.randn(max(SOFT_QS), K, generator=g, device=dev) + 0.8 * rB[t])
        rp = N.pack_codes(rB)
        shape = {"N": n, "bits": K, "bins_soft": 30 * K + 1, "bins_few": 2 * K + 1, "ms": {}}
        for Q in SOFT_QS:
            u = u_all[:Q].contiguous()
            sq, hq = N.soft_query_planes(u), N.pack_codes(torch.sign(u))
            hard = N.soft_query_planes(torch.sign(u))              # every |w| = 15: the Hamming order, wdist = 15 h
            for k in FEW_KS:
                (si, sw), (fi, fd) = N.soft_topk(hard, rp, K, k), N.hamming_topk_few(hq, rp, K, k)
                line["agree_where_they_must"] &= bool(torch.equal(si, fi)) and bool(torch.equal(sw, (30 * fd).to(torch.int32)))
            legs = {"soft_planes": (args.reps, lambda: N.soft_query_planes(u))}
            for k in FEW_KS:
                legs[f"soft_k{k}"] = (args.reps, lambda k=k: N.soft_topk(sq, rp, K, k))
                legs[f"few_k{k}"] = (args.reps, lambda k=k: N.hamming_topk_few(hq, rp, K, k))
            for _, fn in legs.values():                            # warm-up
                fn()
            torch.cuda.synchronize()
            ms = _timed(legs, REGIONS)
            for k in FEW_KS:
                ms[f"soft_k{k}"]["soft_over_few"] = round(ms[f"soft_k{k}"]["median"] / ms[f"few_k{k}"]["median"], 2)
            ms["workspace_mib"] = {"soft": round(N.lib().cmh_soft_topk_workspace_bytes(Q, n, K) / 2 ** 20, 2),
                                   "few": round(N.lib().cmh_topk_few_workspace_bytes(Q, n, K) / 2 ** 20, 2)}
            shape["ms"][f"Q{Q}"] = ms
        line["shapes"][name] = shape
        del rB, rp, u_all
    _emit(args, line)
    if not line["agree_where_they_must"]:
        raise SystemExit("the soft search disagrees with the few-query search on queries whose weights are all 15")


def soft_map_legs(args):
    import torch
    import cmh_native as N
    import utils.retrieval as R
    dev = torch.device("cuda:0")
    for name in args.shapes:
        Q, n, K, C = SHAPES[name]
        g = torch.Generator(device=dev).manual_seed(1)
        rL = (torch.rand(n, C, generator=g, device=dev) < 0.1).float()
        qL = (torch.rand(Q, C, generator=g, device=dev) < 0.1).float()
        rL[:, 0] = 1.0                                            # as map_legs: every query has relevant items, not every pair is relevant
        qL[:, 0] = 1.0
        qL[:, 0][::7] = 0.0
        rL[:, 0][::3] = 0.0
        Wm = torch.randn(C, K, generator=g, device=dev)
        mk = lambda lab: torch.tanh(0.5 * (lab @ Wm) + 0.5 * torch.randn(lab.shape[0], K, generator=g, device=dev) + 1e-3)
        u, rB = mk(qL), torch.sign(mk(rL))
        qp, rp, ql, rl = N.pack_codes(torch.sign(u)), N.pack_codes(rB), N.pack_labels(qL), N.pack_labels(rL)

        def binary():
            s, counts = N.hamming_ap_partial(qp, rp, K, ql, rl, want_counts=True)
            return N.ap_finish(s, counts, K)

        legs = {"soft_map": (1, lambda: R._soft_map("bench", u, rp, K, ql, rl)), "binary": (args.reps, binary)}
        mp, ap, relevant, rank_sum = legs["soft_map"][1]()        # warm-up, and the outputs on the timed inputs
        b_mp, _ = binary()
        rows = 16
        qs, qm, _, _ = N.soft_query_planes(u[:rows].contiguous())
        w = torch.zeros(rows, K, device=dev, dtype=torch.float64)
        for i in range(K):
            bit = ((qm[:, :, i // 32] >> (i % 32)) & 1).double() @ torch.tensor([1.0, 2.0, 4.0, 8.0], device=dev, dtype=torch.float64)
            w[:, i] = bit * (2.0 * ((qs[:, i // 32] >> (i % 32)) & 1).double() - 1.0)
        order = torch.sort(w.abs().sum(1, keepdim=True) - w @ rB.double().T, dim=1, stable=True)[1]
        hits = ((qL[:rows] @ rL.T) > 0).gather(1, order)
        del order
        pos = torch.arange(1, n + 1, device=dev, dtype=torch.float64)
        want = ((hits.cumsum(1).double() / pos) * hits).sum(1) / hits.sum(1).clamp(min=1)
        d_ap = float((ap[:rows].double() - want).abs().max())
        exact = bool(torch.equal(relevant[:rows].long(), hits.sum(1))) and \
            bool(torch.equal(rank_sum[:rows], (hits * torch.arange(1, n + 1, device=dev)).sum(1)))
        auc = R.auc_from_rank_sum(rank_sum, relevant, n)
        del hits, pos, want
        torch.cuda.synchronize()
        line = {"tool": "retrieval_bench", "leg": "soft_map", "shape": name, "Q": Q, "N": n, "bits": K, "classes": C, "regions": REGIONS,
                "blocks": len(R._cuts(Q, N.SOFT_Q_MAX)), "map_soft": float(mp), "map_binary": float(b_mp),
                "mean_auc": float(torch.nanmean(auc)), "max_ap_diff_vs_float64_sort": d_ap, "integers_equal": exact,
                "outputs_equal": exact and d_ap <= 2.4e-7,
                "workspace_mib": round(N.lib().cmh_soft_ap_workspace_bytes(min(Q, N.SOFT_Q_MAX), n, K, ql.shape[1]) / 2 ** 20, 2),
                "ms": _timed(legs, REGIONS)}
        line["ms"]["soft_map"]["soft_over_binary"] = round(line["ms"]["soft_map"]["median"] / line["ms"]["binary"]["median"], 2)
        line["ms"]["soft_map"]["per_block"] = round(line["ms"]["soft_map"]["median"] / line["blocks"], 4)
        _emit(args, line)
        if not line["outputs_equal"]:
            raise SystemExit(f"{name}: the soft mAP by counting disagrees with the float64 AP on a stable sort")
        del u, rB, qp, rp, ql, rl, legs


MASKED_SHARES = (1.0, 0.5, 0.1, 0.01)


def masked_legs(args):
    import torch
    import cmh_native as N
    import utils.retrieval as R
    dev = torch.device("cuda:0")
    line = {"tool": "retrieval_bench", "leg": "masked", "regions": REGIONS, "reps": args.reps, "outputs_equal": True, "shapes": {}}
    for name, (n, K) in FEW.items():
        g = torch.Generator(device=dev).manual_seed(1)
        rB = torch.sign(torch.randn(n, K, generator=g, device=dev) + 1e-3)
        t = torch.randint(0, n, (max(SOFT_QS),), generator=g, device=dev)
        flip = torch.rand(max(SOFT_QS), K, generator=g, device=dev) < 0.1
        qp_all, rp = N.pack_codes(torch.where(flip, -rB[t], rB[t])), N.pack_codes(rB)
        draw = torch.rand(n, generator=g, device=dev)
        del rB, flip
        shape = {"N": n, "bits": K, "ms": {}}
        for Q in SOFT_QS:
            qp = tuple(x[:Q].contiguous() for x in qp_all)
            for k in FEW_KS:
                cell = {}
                for share in MASKED_SHARES:
                    mask = R.ItemMask.from_bool(draw < share)
                    allow = mask.words

                    def gathered(sub=None):
                        keep, rows = sub if sub is not None else (None, None)
                        if sub is None:
                            keep = mask.to_bool().nonzero().flatten()
                            rows = tuple(x.index_select(0, keep) for x in rp)
                        kk = min(k, keep.numel())
                        idx, dist = N.hamming_topk_few(qp, rows, K, kk)
                        return keep[idx.long()].to(torch.int32), dist

                    keep = mask.to_bool().nonzero().flatten()
                    cached = (keep, tuple(x.index_select(0, keep) for x in rp))
                    legs = {"masked": (args.reps, lambda: N.hamming_topk_few_masked(qp, rp, allow, K, k)),
                            "few": (args.reps, lambda: N.hamming_topk_few(qp, rp, K, k)),
                            "gather": (args.reps, gathered),
                            "gather_cached": (args.reps, lambda: gathered(cached))}
                    outs = {leg: fn() for leg, (_, fn) in legs.items()}      # warm-up, and the outputs of both routes on the timed inputs
                    w = outs["gather"][0].shape[1]
                    same = bool(torch.equal(outs["masked"][0][:, :w], outs["gather"][0])) and bool(torch.equal(outs["masked"][1][:, :w], outs["gather"][1])) \
                        and outs["masked"][2].tolist() == [w] * Q and bool((outs["masked"][0][:, w:] == -1).all())
                    if share == 1.0:
                        same = same and bool(torch.equal(outs["masked"][0], outs["few"][0])) and bool(torch.equal(outs["masked"][1], outs["few"][1]))
                    line["outputs_equal"] = line["outputs_equal"] and same
                    del outs
                    torch.cuda.synchronize()
                    ms = _timed(legs, REGIONS)
                    ms["admitted"] = int(keep.numel())
                    ms["masked_over_few"] = round(ms["masked"]["median"] / ms["few"]["median"], 3)
                    ms["gather_over_masked"] = round(ms["gather"]["median"] / ms["masked"]["median"], 2)
                    ms["gather_cached_over_masked"] = round(ms["gather_cached"]["median"] / ms["masked"]["median"], 2)
                    ms["outputs_equal"] = same
                    cell[f"share{share}"] = ms
                    del cached, keep
                shape["ms"][f"Q{Q}_k{k}"] = cell
        line["shapes"][name] = shape
        del qp_all, rp, draw
    _emit(args, line)
    if not line["outputs_equal"]:
        raise SystemExit("the masked search disagrees with the search of the gathered rows")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--reps", type=int, default=5, help="calls per timed region of the new legs")
    ap.add_argument("--out", default="", help="append the JSON lines to this file")
    ap.add_argument("--sharded", action="store_true", help="run the sharded leg (see above) instead of the others")
    ap.add_argument("--map", action="store_true", help="run the mAP legs (see above) instead of the others")
    ap.add_argument("--no-large", action="store_true", help="--map, --rank: leave out the 2 000 000-item database")
    ap.add_argument("--range", action="store_true", help="run the radius-search legs (see above) instead of the others")
    ap.add_argument("--rank", action="store_true", help="run the target-rank legs (see above) instead of the others")
    ap.add_argument("--few", action="store_true", help="run the few-query legs (see above) instead of the others")
    ap.add_argument("--soft", action="store_true", help="run the soft-query legs (see above) instead of the others")
    ap.add_argument("--soft-map", action="store_true", help="run the soft-mAP legs (see above) instead of the others")
    ap.add_argument("--masked", action="store_true", help="run the filtered-search legs (see above) instead of the others")
    args = ap.parse_args()
    import torch
    import cmh_native as N
    if not torch.cuda.is_available():
        raise SystemExit("retrieval_bench needs a GPU: nothing is measured without one")
    if args.sharded:
        return sharded(args)
    if args.map:
        return map_legs(args)
    if args.range:
        return range_legs(args)
    if args.rank:
        return rank_legs(args)
    if args.few:
        return few_legs(args)
    if args.soft:
        return soft_legs(args)
    if args.soft_map:
        return soft_map_legs(args)
    if args.masked:
        return masked_legs(args)
    dev = torch.device("cuda:0")
    for name in args.shapes:
        Q, n, K, C = SHAPES[name]
        g = torch.Generator().manual_seed(1)
        rL = (torch.rand(n, C, generator=g) < 0.1).float()
        qL = (torch.rand(Q, C, generator=g) < 0.1).float()
        rL[:, 0] = 1.0                                            # every query has relevant items: the ranking skips none
        qL[:, 0] = 1.0
        Wm = torch.randn(C, K, generator=g)
        mk = lambda lab: torch.sign(lab @ Wm + 0.5 * torch.randn(lab.shape[0], K, generator=g) + 1e-3).to(dev)
        rp, qp = N.pack_codes(mk(rL)), N.pack_codes(mk(qL))
        rl, ql = N.pack_labels(rL.to(dev)), N.pack_labels(qL.to(dev))
        legs = {
            "ranking": (1, lambda: N.hamming_map(qp, ql, rp, rl, K, C, tie_order=N.TIE_STABLE, want_perm=True)[2][:, :1000]),
            "topk100": (args.reps, lambda: N.hamming_topk(qp, rp, K, 100, ql, rl)),
            "topk1000": (args.reps, lambda: N.hamming_topk(qp, rp, K, 1000, ql, rl)),
            "hist": (args.reps, lambda: N.hamming_hist(qp, rp, K, ql, rl)),
            "graded100": (args.reps, lambda: N.hamming_topk_graded(qp, rp, K, 100, ql, rl, classes=C)),
            "graded1000": (args.reps, lambda: N.hamming_topk_graded(qp, rp, K, 1000, ql, rl, classes=C)),
            "labelhist": (args.reps, lambda: N.label_overlap_hist(ql, rl, C)),
        }
        # warm-up, and the outputs of the two routes on the timed inputs
        perm = legs["ranking"][1]()
        i100, i1000, counts = legs["topk100"][1](), legs["topk1000"][1](), legs["hist"][1]()
        same = bool(torch.equal(i1000[0], perm)) and bool(torch.equal(i100[0], perm[:, :100]))
        full = N.hamming_dist((qp[0][:64].contiguous(), qp[1][:64].contiguous()), rp, K)
        same = same and bool(torch.equal(i1000[1][:64], full.gather(1, i1000[0][:64].long())))
        same = same and bool((counts.long().sum((1, 2)) == n).all())
        g100, g1000, gcounts = legs["graded100"][1](), legs["graded1000"][1](), legs["labelhist"][1]()
        graded_same = all(bool(torch.equal(a[j], b[j])) for a, b in ((g100, i100), (g1000, i1000)) for j in (0, 1))
        graded_same = graded_same and bool(torch.equal((g1000[2] > 0).to(torch.uint8), i1000[2]))
        graded_same = graded_same and bool(torch.equal(n - gcounts[:, 0], counts[:, :, 1].sum(1).to(gcounts.dtype)))
        del perm, full, g100, g1000, gcounts
        torch.cuda.synchronize()
        times = {k: [] for k in legs}
        for _ in range(REGIONS):
            for leg, (reps, fn) in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    out = fn()
                e1.record()
                e1.synchronize()
                del out
                times[leg].append(e0.elapsed_time(e1) / reps)
        line = {"tool": "retrieval_bench", "shape": name, "Q": Q, "N": n, "bits": K, "classes": C, "regions": REGIONS,
                "outputs_equal": same, "graded_outputs_equal": graded_same, "ms": {}}
        for leg, ts in times.items():
            line["ms"][leg] = {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}
        for leg, passes in (("topk100", 2), ("topk1000", 2), ("hist", 1)):
            fl = floors_ms(Q, n, K, C, passes)
            line["ms"][leg]["floor_ms"] = {k: (round(v, 4) if k != "bound" else v) for k, v in fl.items()}
            line["ms"][leg]["share_of_floor"] = round(fl[fl["bound"]] / line["ms"][leg]["median"], 4)
            line["ms"][leg]["ranking_min_over_max"] = round(line["ms"]["ranking"]["min"] / line["ms"][leg]["max"], 2)
        for leg, base in (("graded100", "topk100"), ("graded1000", "topk1000")):
            line["ms"][leg]["graded_over_plain"] = round(line["ms"][leg]["median"] / line["ms"][base]["median"], 4)
        line["ms"]["labelhist"]["labelhist_over_hist"] = round(line["ms"]["labelhist"]["median"] / line["ms"]["hist"]["median"], 4)
        line["new_slowest_beats_ranking_fastest"] = all(line["ms"][leg]["max"] < line["ms"]["ranking"]["min"] for leg in ("topk100", "topk1000"))
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(text + "\n")
        if not same:
            raise SystemExit(f"{name}: the two routes disagree")
        if not graded_same:
            raise SystemExit(f"{name}: the graded search disagrees with the plain search")


if __name__ == "__main__":
    main()
