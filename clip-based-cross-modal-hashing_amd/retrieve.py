"""Top-k search in the codes a trainer saved: serves the PR_cruve/<bits>-ours-<dataset>-<mode>.mat files of TrainBase.save_mat
(q_img q_txt r_img r_txt q_l r_l), no model needed.

    python retrieve.py --codes result/DSPH/flickr25k/64/PR_cruve/64-ours-flickr25k-i2t.mat --direction i2t --k 10 --queries 0:5

prints one line per query: its number, then `index:distance` (`index:distance:hit` when the file has labels) for the k nearest
database items, nearest first, ties by database index.  With --graded the third field is the number of labels the neighbour shares
with the query (0 = no hit) instead of the 0/1 flag.

    python retrieve.py --codes <file>.mat --index db.npz --direction i2t --k 10

searches a saved CodeIndex (CodeIndex.save: any number of items, grown by CodeIndex.add) in place of the .mat's database side; the
.mat still supplies the queries (the query side of --direction) and their labels.  The database half of --direction is then unused;
a note on stderr says so when the file holds that side.

    python retrieve.py --codes <file>.mat --direction i2t --map [--k K]

prints one line, the mAP (mAP@K with --k) of the chosen direction over the file's queries (--queries) against the database side or
--index, ties by ascending database index, for a database of any size.  It needs labels (q_l, r_l).

    python retrieve.py --codes <file>.mat --direction i2t --radius 2 [--max-hits M]

prints one line per query: its number, then `index:distance` (`index:distance:hit` with labels) for EVERY database item within
Hamming radius R (the units of the distance column; 0.5 steps count for codes with zeros), nearest first, ties by database index.  A
query whose ball is empty prints its number alone.  --radius excludes --k, --map and --graded; more than --max-hits entries over
all queries are refused before they are allocated.

    python retrieve.py --codes <file>.mat --direction i2t --recall [--ks 1,5,10] [--ties index|optimistic|pessimistic|expected]

prints one line, `R@1: ... R@5: ... R@10: ... MedR: ... MeanR: ... MRR: ...`: where the item that BELONGS to each query ranks
(instance-level recall, by counting: any database size).  The database is the QUERY side of the direction's other modality (i2t:
q_img against q_txt, the paired test-set protocol) and query i belongs to item i; --queries slices the queries and their targets
with them.  With --index the database is the saved index and --targets FILE names the pairing: one line per query of the file
(before --queries), holding the space-separated database indices that belong to it; an empty line = no target.  --ties picks the
order inside a group of equal distances (index: by database index, as every other mode here; expected: the mean over random
orders, without MRR).  --recall excludes --radius, --map, --graded and --k.

    python retrieve.py --text "a dog on a beach" --index db.npz --method DSPH --pretrained model.pth -clip-path ViT-B-32.pt --output-dim 64 --k 10

asks the index a question: every --text CAPTION and --image PATH (both repeatable, in any mix; answered in the order given) is
encoded by the trained model (query.py::QueryEncoder: the tokenizer or the image transform, the towers, the method's heads and its
code rule) and searched in the saved CodeIndex.  No --codes file is needed.  Per query one block: a line `query <number> <text|image>:
<what was asked>`, then k lines `<rank> <database index> <distance>`, nearest first, ties by database index.  --max-words,
--resolution, --gemm-dtype and --bpe-path are the trainer's options of those names.  MITH and TwDH are not supported here.

    python retrieve.py --text "a dog on a beach" --soft --index db.npz --method DSPH --pretrained model.pth -clip-path ViT-B-32.pt --output-dim 64

ranks by the model's real-valued output instead of its sign (CodeIndex.search_soft: the asymmetric distance, which orders the items
a Hamming ranking leaves tied); the same blocks, the distance column in the soft distance's units.  --soft goes with --text /
--image only.

    python retrieve.py --text "a dog on a beach" --index db.npz ... --any-label 3,7 --no-label 2 --exclude-ids seen.txt

filters the search: only the items of the index that carry at least one of the classes of --any-label, all of --all-labels and none
of --no-label (class numbers, comma-separated; the index must hold labels), that are listed in --only-ids FILE and not listed in
--exclude-ids FILE (one database index per line) are searched; the conditions given combine by AND.  The filters go with --index in
the neighbour modes (--text / --image, also with --soft, and --codes --index), not with --map, --graded, --radius or --recall.  The
indices printed are the index's own.  A query with fewer than --k admitted items prints only those it found.

    python retrieve.py --codes <file>.mat --stats [--stats-out stats.npz]
    python retrieve.py --index db.npz --stats

prints the code diagnostics (utils/code_stats.py) in place of a search: per modality (r_img, r_txt; with --index the index alone) the
bit balance, the dead and duplicated bits, the mean and largest |correlation| between two bits with the pair that has it; for the
.mat's pairing (database image i <-> caption i) the mean agreement of the two codes and the three bits that agree least; with labels
(r_l, or an index that holds some) per bit the class it tells most about, as bit:class:mutual information.  --stats-out stores
every array, the integers behind them included, as one .npz.  --stats excludes --map, --radius, --recall, --text and --image.

    python retrieve.py --codes <file>.mat --direction i2t --lookup 2 [--queries a:b]

prints what --radius 2 prints, line for line, from the index's bucket table (CodeIndex.lookup: the database items grouped by equal
code, each query's ball found by key at a cost that does not grow with the database).  R is 0, 1 or 2 whole bits; codes up to 128
bit without zero entries (--radius takes the others).  --lookup excludes --radius, --k, --map, --graded, --recall, --soft, --stats
and the filters.

    python retrieve.py --codes <file>.mat --bucket-stats [--stats-out buckets.npz]
    python retrieve.py --index db.npz --bucket-stats

prints, per database side (r_img, r_txt; with --index the index alone), how the items spread over their distinct codes: the distinct
codes, the singletons, the largest bucket, the share of the possible codes in use, the colliding pairs, the collision probability
and the entropy of the bucket sizes.  --stats-out stores the numbers and the (size, buckets) occupancy tables; with --stats both
reports are printed and stored.  The exclusions are those of --stats.

    python retrieve.py --codes <file>.mat --direction i2t --near 4 [--index db.npz] [--queries a:b]

prints what --radius 4 prints, line for line, from the index's substring tables (CodeIndex.lookup_far: multi-index hashing on 16-bit
substrings, the candidates verified with the full distance).  R is a whole number of bits up to 3 ceil(bits / 16) - 1 (11 at 64
bit, 23 at 128); codes up to 128 bit without zero entries (--radius takes the others).  --near excludes what --lookup excludes,
and --lookup.

    python retrieve.py --codes <file>.mat --direction i2t --k 10 --tables [--index db.npz] [--queries a:b]
    python retrieve.py --text "a dog on a beach" --tables --index db.npz --method DSPH ... --k 10

prints what the same command prints without --tables, line for line, from the index's substring tables (CodeIndex.search_tables:
every query's radius grown until its ball holds k items; a query whose ball is too wide, or not within 3 ceil(bits / 16) - 1 bits,
is answered by the scan).  Codes up to 128 bit without zero entries.  --tables excludes --soft, the filters, --graded, --radius,
--lookup, --near, --map, --recall, --stats and --bucket-stats."""
import argparse
import sys

DIRECTIONS = {"i2t": ("q_img", "r_txt"), "t2i": ("q_txt", "r_img"), "i2i": ("q_img", "r_img"), "t2t": ("q_txt", "r_txt")}
TIES = ("index", "optimistic", "pessimistic", "expected")
LABEL_FILTERS = ("--any-label", "--all-labels", "--no-label")
FILTERS = LABEL_FILTERS + ("--only-ids", "--exclude-ids")


class _Ask(argparse.Action):
    """--text / --image append (kind, value) to one list, so that the questions keep the order of the command line."""

    def __call__(self, parser, namespace, value, option_string=None):
        namespace.ask = (getattr(namespace, "ask", None) or []) + [(option_string.lstrip("-"), value)]


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--codes", default=None, help=".mat file written by a trainer (save_mat); required unless --text / --image ask the questions")
    p.add_argument("--text", action=_Ask, metavar="CAPTION", help="search the --index for this caption (repeatable; needs --method, --pretrained, -clip-path, --output-dim)")
    p.add_argument("--image", action=_Ask, metavar="PATH", help="search the --index for this picture (repeatable, mixes with --text)")
    p.add_argument("--soft", action="store_true", help="with --text / --image: rank by the model's real-valued output (soft queries) instead of its sign")
    p.add_argument("--method", default=None, help="with --text / --image: the method the checkpoint was trained with")
    p.add_argument("--pretrained", default=None, metavar="FILE", help="with --text / --image: the trained model (model-<epoch>.pth)")
    p.add_argument("-clip-path", "--clip-path", dest="clip_path", default=None, metavar="FILE", help="with --text / --image: the CLIP checkpoint the model was built on")
    p.add_argument("--output-dim", type=int, default=None, help="with --text / --image: the code length in bits")
    p.add_argument("--max-words", type=int, default=32)
    p.add_argument("--resolution", type=int, default=224)
    p.add_argument("--gemm-dtype", default="f32")
    p.add_argument("--bpe-path", default=None, metavar="FILE", help="the CLIP BPE merges file (default: next to the tokenizer)")
    p.add_argument("--direction", choices=sorted(DIRECTIONS), default="i2t", help="query side -> database side")
    p.add_argument("--k", type=int, default=None, help="neighbours per query (default 10); with --map: mAP@K (default: the whole database)")
    p.add_argument("--map", action="store_true", help="print the mAP of the direction in place of the neighbours (needs labels in the file)")
    p.add_argument("--queries", default=":", help="slice a:b of the file's queries (default: all)")
    p.add_argument("--index", default="", metavar="FILE", help="a saved CodeIndex (.npz of CodeIndex.save) as the database, in place of the .mat's database side")
    p.add_argument("--graded", action="store_true", help="print the shared-label count of each neighbour in place of the hit flag (needs labels in the file)")
    p.add_argument("--radius", type=float, default=None, metavar="R", help="print every database item within Hamming radius R of each query in place of the k nearest")
    p.add_argument("--max-hits", type=int, default=None, metavar="M", help="with --radius: refuse more than M entries in all (default 2^31 - 1)")
    p.add_argument("--recall", action="store_true", help="print Recall@K, MedR, mean rank and MRR of the item that belongs to each query in place of the neighbours")
    p.add_argument("--ks", default=None, metavar="K1,K2,...", help="with --recall: the cut-offs (default 1,5,10)")
    p.add_argument("--ties", choices=TIES, default=None, help="with --recall: the order inside a group of equal distances (default index)")
    p.add_argument("--targets", default=None, metavar="FILE", help="with --recall --index: one line per query, the database indices that belong to it")
    p.add_argument("--any-label", default=None, metavar="C1,C2,...", help="with --index: only items that carry at least one of these classes")
    p.add_argument("--all-labels", default=None, metavar="C1,C2,...", help="with --index: only items that carry all of these classes")
    p.add_argument("--no-label", default=None, metavar="C1,C2,...", help="with --index: only items that carry none of these classes")
    p.add_argument("--only-ids", default=None, metavar="FILE", help="with --index: only the database indices listed in FILE, one per line")
    p.add_argument("--exclude-ids", default=None, metavar="FILE", help="with --index: not the database indices listed in FILE, one per line")
    p.add_argument("--stats", action="store_true", help="print the code diagnostics of the file's database sides (or of --index) in place of a search")
    p.add_argument("--stats-out", default=None, metavar="FILE", help="with --stats / --bucket-stats: store every array as FILE (.npz)")
    p.add_argument("--lookup", type=int, default=None, metavar="R", help="print every database item within R = 0, 1 or 2 bits of each query, as --radius does, from the index's bucket table")
    p.add_argument("--bucket-stats", action="store_true", help="print how the items of the file's database sides (or of --index) spread over their distinct codes in place of a search")
    p.add_argument("--near", type=int, default=None, metavar="R", help="print every database item within R whole bits of each query, as --radius does, from the index's substring tables (R up to 3 ceil(bits / 16) - 1)")
    p.add_argument("--tables", action="store_true", help="find the k nearest through the index's substring tables (the radius grown per query) in place of the scan: the same lines")
    args = p.parse_args(argv)
    args.ask = getattr(args, "ask", None) or []
    if args.tables:
        for flag, given in (("--soft", args.soft), ("--graded", args.graded), ("--radius", args.radius is not None),
                            ("--lookup", args.lookup is not None), ("--near", args.near is not None), ("--map", args.map),
                            ("--recall", args.recall), ("--stats", args.stats), ("--bucket-stats", args.bucket_stats)) \
                + tuple((f, getattr(args, f[2:].replace("-", "_")) is not None) for f in FILTERS):
            if given:
                p.error(f"--tables and {flag} exclude each other")
    if args.near is not None:
        for flag, given in (("--radius", args.radius is not None), ("--lookup", args.lookup is not None), ("--k", args.k is not None),
                            ("--map", args.map), ("--graded", args.graded), ("--recall", args.recall), ("--soft", args.soft),
                            ("--stats", args.stats), ("--bucket-stats", args.bucket_stats), ("--text / --image", bool(args.ask))) \
                + tuple((f, getattr(args, f[2:].replace("-", "_")) is not None) for f in FILTERS):
            if given:
                p.error(f"--near and {flag} exclude each other")
        if args.near < 0:
            p.error(f"--near {args.near}: a whole number of bits >= 0 (--radius takes any radius)")
    if args.lookup is not None:
        for flag, given in (("--radius", args.radius is not None), ("--k", args.k is not None), ("--map", args.map), ("--graded", args.graded),
                            ("--recall", args.recall), ("--soft", args.soft), ("--stats", args.stats), ("--bucket-stats", args.bucket_stats),
                            ("--text / --image", bool(args.ask))) + tuple((f, getattr(args, f[2:].replace("-", "_")) is not None) for f in FILTERS):
            if given:
                p.error(f"--lookup and {flag} exclude each other")
        if not 0 <= args.lookup <= 2:
            p.error(f"--lookup {args.lookup}: 0, 1 or 2 bits (--radius takes any radius)")
    for name, on in (("--stats", args.stats), ("--bucket-stats", args.bucket_stats)):
        if not on:
            continue
        for flag, given in (("--map", args.map), ("--radius", args.radius is not None), ("--recall", args.recall),
                            ("--text / --image", bool(args.ask))):
            if given:
                p.error(f"{name} and {flag} exclude each other")
        if args.codes is None and not args.index:
            p.error(f"{name}: --codes FILE or --index FILE is required")
    if args.stats_out is not None and not (args.stats or args.bucket_stats):
        p.error("--stats-out goes with --stats")
    args.filtered = False
    for flag in FILTERS:
        value = getattr(args, flag[2:].replace("-", "_"))
        if value is None:
            continue
        args.filtered = True
        if not args.index:
            p.error(f"{flag} filters a saved CodeIndex: --index FILE is required")
        for other, given in (("--map", args.map), ("--graded", args.graded), ("--recall", args.recall), ("--radius", args.radius is not None)):
            if given:
                p.error(f"{flag} and {other} exclude each other (a filter goes with the neighbour modes)")
        if flag in LABEL_FILTERS:
            try:
                classes = [int(c) for c in value.split(",")]
            except ValueError:
                classes = [-1]
            if min(classes) < 0:
                p.error(f"{flag}: comma-separated class numbers >= 0")
            setattr(args, flag[2:].replace("-", "_"), classes)
    if args.ask:
        if not args.index:
            p.error("--text / --image search a saved CodeIndex: --index FILE is required")
        for flag, given in (("--codes", args.codes is not None), ("--map", args.map), ("--graded", args.graded), ("--recall", args.recall),
                            ("--radius", args.radius is not None), ("--queries", args.queries != ":")):
            if given:
                p.error(f"--text / --image and {flag} exclude each other")
        missing = [flag for flag, v in (("--method", args.method), ("--pretrained", args.pretrained), ("-clip-path", args.clip_path),
                                        ("--output-dim", args.output_dim)) if v is None]
        if missing:
            p.error(f"--text / --image need the model: {', '.join(missing)} missing")
        if args.k is not None and args.k < 1:
            p.error("--k: at least 1")
    elif args.soft:
        p.error("--soft goes with --text / --image: a soft query is the model's output, a --codes file holds only signs")
    elif args.codes is None and not (args.stats or args.bucket_stats):
        p.error("the following arguments are required: --codes")
    if args.recall:
        for flag, given in (("--radius", args.radius is not None), ("--map", args.map), ("--graded", args.graded), ("--k", args.k is not None)):
            if given:
                p.error(f"--recall and {flag} exclude each other")
        if bool(args.index) != (args.targets is not None):
            p.error("--recall: --index and --targets go together (without them the pairing is the identity over the file's query sides)")
        try:
            args.ks = [int(k) for k in ("1,5,10" if args.ks is None else args.ks).split(",")]
        except ValueError:
            args.ks = []
        if not args.ks or min(args.ks) < 1:
            p.error("--ks: comma-separated integers >= 1")
        args.ties = args.ties or "index"
    else:
        for flag, given in (("--ks", args.ks is not None), ("--ties", args.ties is not None), ("--targets", args.targets is not None)):
            if given:
                p.error(f"{flag} goes with --recall")
    if args.radius is not None:
        for flag, given in (("--k", args.k is not None), ("--map", args.map), ("--graded", args.graded)):
            if given:
                p.error(f"--radius and {flag} exclude each other")
        if args.radius != args.radius or args.radius < 0:
            p.error(f"--radius {args.radius}: a number >= 0")
    elif args.max_hits is not None:
        p.error("--max-hits goes with --radius")
    return args


def query_slice(text, n):
    a, _, b = text.partition(":")
    lo, hi = (int(a) if a else 0), (int(b) if b else n)
    if not 0 <= lo <= hi <= n:
        raise SystemExit(f"--queries {text}: outside 0:{n}")
    return lo, hi


def read_targets(path, queries, items):
    """One line per query: the space-separated database indices that belong to it -> int64 [queries, G], -1 = padding."""
    import torch
    with open(path) as f:
        rows = [[int(x) for x in line.split()] for line in f.read().splitlines()]
    if len(rows) != queries:
        raise SystemExit(f"--targets {path}: {len(rows)} lines for {queries} queries")
    if any(not 0 <= t < items for r in rows for t in r):
        raise SystemExit(f"--targets {path}: an index outside 0..{items - 1}")
    G = max(1, max(len(r) for r in rows))
    return torch.tensor([r + [-1] * (G - len(r)) for r in rows], dtype=torch.int64).reshape(queries, G)


def read_ids(flag, path, items):
    """One database index per line (blank lines are skipped) -> a list of integers inside the index."""
    try:
        with open(path) as f:
            ids = [int(line) for line in f.read().split()]
    except (OSError, ValueError) as e:
        raise SystemExit(f"{flag} {path}: {e}")
    if any(not 0 <= i < items for i in ids):
        raise SystemExit(f"{flag} {path}: an index outside 0..{items - 1}")
    return ids


def item_mask(args, index):
    """The ItemMask of the filter options over the index; None when none is given."""
    if not args.filtered:
        return None
    if index.labels is None and (args.any_label is not None or args.all_labels is not None or args.no_label is not None):
        raise SystemExit(f"--index {args.index} holds no labels: --any-label / --all-labels / --no-label cannot filter it")
    for flag, classes in (("--any-label", args.any_label), ("--all-labels", args.all_labels), ("--no-label", args.no_label)):
        if classes is not None and max(classes) >= index.classes:
            raise SystemExit(f"{flag}: the index holds classes 0..{index.classes - 1}")
    return index.mask(any_of=args.any_label, all_of=args.all_labels, none_of=args.no_label,
                      ids=None if args.only_ids is None else read_ids("--only-ids", args.only_ids, index.size),
                      exclude_ids=None if args.exclude_ids is None else read_ids("--exclude-ids", args.exclude_ids, index.size))


def recall(args, m, q_key, r_key, lo, hi):
    import torch

    from utils.retrieval import CodeIndex
    if hi == lo:
        raise SystemExit("--recall: no queries")
    queries = torch.from_numpy(m[q_key][lo:hi]).float()
    if args.index:
        index = CodeIndex.load(args.index)
        targets = read_targets(args.targets, m[q_key].shape[0], index.size)[lo:hi]
    else:
        side = "q_" + r_key[2:]                                    # the query side of the other modality: the paired items
        index = CodeIndex(torch.from_numpy(m[side]).float())
        targets = torch.arange(lo, hi)
    if index.bits != queries.shape[1]:
        raise SystemExit(f"--recall: {index.bits}-bit database codes, the queries of {args.codes} have {queries.shape[1]}")
    out = index.recall(queries, targets, ks=args.ks, ties=args.ties)
    cols = [f"R@{k}: {float(v):.6f}" for k, v in zip(args.ks, out["recall"])]
    cols += [f"MedR: {out['median_rank']:g}", f"MeanR: {out['mean_rank']:.6f}"] + ([f"MRR: {out['mrr']:.6f}"] if "mrr" in out else [])
    print(" ".join(cols))
    return 0


def stats(args):
    """--stats: the diagnostics of the index, or of both database sides of the .mat and their pairing.  --bucket-stats: how the
    items of the same sides spread over their distinct codes."""
    import numpy as np
    import torch

    from utils import code_stats as S
    from utils.retrieval import CodeIndex
    sides, indexes = {}, {}
    if args.index:
        indexes["index"] = CodeIndex.load(args.index)
        if args.stats:
            sides = {"index": S.code_stats(indexes["index"])}
    else:
        import scipy.io as scio
        m = scio.loadmat(args.codes)
        labels = torch.from_numpy(m["r_l"]).float() if "r_l" in m else None
        img, txt = (torch.from_numpy(m[k]).float() if k in m else None for k in ("r_img", "r_txt"))
        if img is None and txt is None:
            raise SystemExit(f"--stats: {args.codes} holds neither r_img nor r_txt")
        paired = img is not None and txt is not None and img.shape[0] == txt.shape[0]
        if args.stats:
            sides = {name: S.code_stats(own, labels=labels, paired=other if paired else None)
                     for name, own, other in (("r_img", img, txt), ("r_txt", txt, img)) if own is not None}
        if args.bucket_stats:
            indexes = {name: CodeIndex(own) for name, own in (("r_img", img), ("r_txt", txt)) if own is not None}
    out = {}
    for i, (name, st) in enumerate(sides.items()):
        if i:                                                      # the pairing is one fact: shown with the first side
            st = {k: v for k, v in st.items() if k != "bit_agreement"}
        print("\n".join(S.summary_lines(name, st)))
        out.update(S.arrays(sides[name], name + "_"))
    if args.bucket_stats:
        import cmh_native as N
        for name, index in indexes.items():
            try:
                st = index.bucket_stats()
            except N.NativeError as e:                             # codes with zeros have no bucket table
                raise SystemExit(f"--bucket-stats: {name}: {e}")
            print("\n".join(S.bucket_summary_lines(name, st)))
            out.update({f"{name}_bucket_{k}": np.asarray(v) for k, v in st.items()})
    if args.stats_out:
        with open(args.stats_out, "wb") as f:
            np.savez(f, **out)
    return 0


def search_tables(index, queries, k, labels):
    """--tables: CodeIndex.search_tables, its refusals (zeros in the codes, more than 128 bits) as the command's."""
    import cmh_native as N
    try:
        return index.search_tables(queries, k, labels)
    except N.NativeError as e:
        raise SystemExit(f"--tables: {e}")


def ask(args):
    """--text / --image: encode the questions, search the index, print one block per question."""
    from query import QueryEncoder, check_method
    try:
        check_method(args.method)                                  # by name, before the index or the checkpoint is read
    except (NotImplementedError, ValueError) as e:
        raise SystemExit(str(e))
    import torch

    from utils.retrieval import CodeIndex
    index = CodeIndex.load(args.index)
    if index.bits != args.output_dim:
        raise SystemExit(f"--index {args.index}: {index.bits}-bit codes, the model of --output-dim {args.output_dim} writes {args.output_dim}-bit ones")
    enc = QueryEncoder(args.method, args.pretrained, args.clip_path, args.output_dim, max_words=args.max_words,
                       resolution=args.resolution, gemm_dtype=args.gemm_dtype, bpe_path=args.bpe_path)
    k = min(10 if args.k is None else args.k, index.size)
    texts = [v for kind, v in args.ask if kind == "text"]
    images = [v for kind, v in args.ask if kind == "image"]
    codes = {"text": enc.encode_text(texts, soft=args.soft) if texts else None,
             "image": enc.encode_image(images, soft=args.soft) if images else None}
    at = {"text": 0, "image": 0}
    rows = []
    for kind, _ in args.ask:                                       # back into the order of the command line
        rows.append(codes[kind][at[kind]])
        at[kind] += 1
    mask = item_mask(args, index)
    if args.tables:
        got = search_tables(index, torch.stack(rows), k, None)
    else:
        got = index.search_soft(torch.stack(rows), k, mask=mask) if args.soft else index.search(torch.stack(rows), k, mask=mask)
    idx, dist = (t.cpu().numpy() for t in got[:2])
    count = [k] * len(rows) if mask is None else got[3].cpu().tolist()      # a filtered row holds only what the filter admits
    for i, (kind, value) in enumerate(args.ask):
        print(f"query {i} {kind}: {value}")
        for j in range(count[i]):
            print(f"{j + 1} {idx[i, j]} {dist[i, j]:g}")
    return 0


def main(argv=None):
    args = parse(argv)
    if args.ask:
        return ask(args)
    if args.stats or args.bucket_stats:
        return stats(args)
    import scipy.io as scio
    import torch

    from utils.retrieval import CodeIndex
    q_key, r_key = DIRECTIONS[args.direction]
    m = scio.loadmat(args.codes)
    lo, hi = query_slice(args.queries, m[q_key].shape[0])
    if args.recall:
        return recall(args, m, q_key, r_key, lo, hi)
    index = CodeIndex.load(args.index) if args.index else CodeIndex.from_mat(args.codes, side=r_key)
    if args.index and r_key in m:
        print(f"note: --index {args.index} is the database; {r_key} of {args.codes} (--direction {args.direction}) is not searched, "
              f"only its query side {q_key} is used", file=sys.stderr)
    if index.bits != m[q_key].shape[1]:
        raise SystemExit(f"--index {args.index}: {index.bits}-bit codes, the queries of {args.codes} have {m[q_key].shape[1]}")
    queries = torch.from_numpy(m[q_key][lo:hi]).float()
    labels = torch.from_numpy(m["q_l"][lo:hi]).float() if index.labels is not None and "q_l" in m else None
    if args.graded and labels is None:
        raise SystemExit(f"--graded: {args.codes} holds no labels (q_l, r_l)")
    if args.map:
        if labels is None:
            raise SystemExit(f"--map: needs labels (q_l of {args.codes} and the database's)")
        if hi == lo:
            raise SystemExit("--map: no queries")
        print(f"{float(index.map(queries, labels, k=args.k)):.8f}")
        return 0
    if hi == lo:
        return 0
    if args.radius is not None or args.lookup is not None or args.near is not None:
        if args.lookup is not None or args.near is not None:
            import cmh_native as N
            try:
                found = index.lookup(queries, args.lookup, labels) if args.near is None else index.lookup_far(queries, args.near, labels)
                out = [t.cpu().numpy() for t in found]
            except N.NativeError as e:                             # zeros in the codes, more than 128 bits, a radius beyond the tables': --radius takes them
                raise SystemExit(f"{'--lookup' if args.near is None else '--near'}: {e}")
        else:
            out = [t.cpu().numpy() for t in index.range_search(queries, args.radius, labels, max_hits=args.max_hits)]
        for i in range(hi - lo):
            cols = [f"{out[1][j]}:{out[2][j]:g}" + (f":{out[3][j]}" if len(out) == 4 else "") for j in range(out[0][i], out[0][i + 1])]
            print(" ".join([str(lo + i)] + cols))
        return 0
    args.k = 10 if args.k is None else args.k
    mask = item_mask(args, index)
    count = [args.k] * (hi - lo)
    if args.tables:
        out = [t.cpu().numpy() for t in search_tables(index, queries, args.k, labels)]
    elif mask is None:
        out = [t.cpu().numpy() for t in index.search(queries, args.k, labels, graded=args.graded)]
    else:
        idx, dist, rel, found = index.search(queries, args.k, labels, mask=mask)
        out = [t.cpu().numpy() for t in (idx, dist) + (() if rel is None else (rel,))]
        count = found.cpu().tolist()                               # a filtered row holds only what the filter admits
    for i in range(hi - lo):
        cols = [f"{out[0][i, j]}:{out[1][i, j]:g}" + (f":{out[2][i, j]}" if len(out) == 3 else "") for j in range(count[i])]
        print(lo + i, " ".join(cols))
    return 0


if __name__ == "__main__":
    sys.exit(main())
