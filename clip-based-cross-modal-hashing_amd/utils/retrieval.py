"""Retrieval with the hash codes on libcmh.so (csrc/retrieval.hip): top-k Hamming search and the two curves every paper behind the
built methods reports next to mAP, precision-recall by Hamming radius and top-N precision.  The reference leaves them to an offline
step on the .mat files of train/base.py::save_mat; here they run on the GPU from the packed codes.

Inputs are what calc_utils.py takes: f32 codes in {-1, 0, +1} and f32 multi-hot labels on any device.  Distances are
calc_hammingDist's (utils/calc_utils.py:8-13), relevance is calc_neighbor's test (:42-45), ties are ordered by ascending database
index (torch.sort(stable=True)).

Conventions of the curves:
  * means run over the queries that have at least one relevant database item; the others are left out of numerator and denominator
    (mAP differs: the reference divides by all queries);
  * the precision of an empty ball is 0;
  * recall = hits / relevant items in the database.
The integer counts / hit flags come back too, so a caller who shards queries over ranks, or wants another convention, sums them.
The Q x N work runs in the kernels; reducing counts to curves is float64 arithmetic on small CPU tensors.

Graded relevance (the multi-label numbers next to mAP: NDCG@n, ACG@n, WAP@n).  The grade of a pair is the NUMBER of labels it
shares, g(q, j) = popcount(packed_label(q) & packed_label(j)) = (query_L @ retrieval_L.T)[q, j] for 0/1 labels: the matrix that
calc_neighbor thresholds.  With g_i the grade of the item at position i (1-based) of a query's ranking (the order of hamming_topk):
  ACG@n  = (1/n) sum_{i<=n} g_i
  DCG@n  = sum_{i<=n} (2^g_i - 1) / log2(i + 1);   IDCG@n = the same sum over the database's grades in descending order
  NDCG@n = DCG@n / IDCG@n
  WAP@n  = (1/R_n) sum_{i<=n, g_i>0} ACG@i,   R_n = #{i <= n : g_i > 0};   WAP@n = 0 if R_n = 0
Means follow the convention of the curves: over the queries with at least one relevant database item (the others have IDCG = 0).
graded_topk returns the grades of the neighbours; grade_histogram counts, per query, the database items of every grade (it depends
on the labels only: one call serves all directions of an evaluation) and is what IDCG is computed from, without sorting anything.

Few queries (Q <= QUERIES_FEW, k <= 4096, codes up to 128 bit, no shard size stated) take ONE cmh_hamming_topk_few over the whole
database, whatever its size (csrc/retrieval_few.hip: lanes own items; _few_route): the same bytes as the route below.

Soft queries.  soft_topk / CodeIndex.search_soft rank the database by the head's REAL-VALUED output u (query.py: encode_*(...,
soft=True); code_rules.SOFT_RULES) in place of its sign: calc_hammingDist on u, the asymmetric distance, which orders the items a
Hamming ranking leaves tied.  u is quantised per row to integer weights w_i = rint((u_i / max|u|) * 15) and the database stays the
packed planes: wdist = sum |w_i| - sum w_i r_i (an exact integer), dist = wdist * (max|u| / 30) = 0.5 (sum |u~_i| - u~ . r) for
the quantised query u~, ties by ascending database index.  One cmh_soft_topk (csrc/retrieval_soft.hip) per block of 64 queries
over the whole database, whatever its size; codes up to 128 bit and k <= 4096, and no other route computes this distance.

Filtered search.  hamming_topk / soft_topk / CodeIndex.search / CodeIndex.search_soft take mask=ItemMask: the nearest items AMONG
THOSE the mask admits (items that carry a label, that are not in a deny list, an id range ...), with database indices, and without
a packed copy of the admitted rows.  An ItemMask is one bit per database item (int64 words, bit j % 64 of word j / 64); it is made
from booleans, id lists or label conditions (ItemMask.from_*, CodeIndex.mask) and combined with & | ~.  A masked search always
takes the few-query kernels (cmh_hamming_topk_few_masked / cmh_soft_topk_masked: one 64-bit word per 64 items in the walk), in
blocks of 64 queries, and returns one more element, found int32 [Q] = min(k, admitted items): the columns at and behind found[q]
are pads (idx = -1, dist = +inf, rel = 0, wdist = 2^31 - 1).  k is checked against the database, not against the admitted count
(that lives on the GPU; nothing synchronises).  Codes up to 128 bit and k <= 4096; the tiles route (shards, grades, histograms)
takes no mask.

Size.  The other native entry points take N <= 524 287 database items and Q <= 65 535 queries per call.  Every function here takes any
database up to 2^31 - 1 items and any number of queries: the packed planes are row-major, so the database is cut into SHARDS of
`shard_items` rows (views, packed once), every shard is searched, and the per-shard lists are folded together in ascending shard
order by cmh_topk_merge (csrc/retrieval_merge.hip), which keeps the order (distance, database index): the result is bit for bit
what one search over the whole database would give.  Histograms are the int32 sums of the per-shard histograms; queries are cut
into blocks of QUERIES_MAX rows and the outputs concatenated.  A database and a query set within the limits take exactly one
native call.  CodeIndex grows by add() and persists by save() / load().

mAP.  mean_average_precision is calc_map_k_matrix's number with ties by ascending database index, computed by counting
(cmh_hamming_ap_partial): a relevant item's rank is a sum of histogram entries and of a cursor, so nothing is sorted and the
shards' float64 sums add.  It is the only mAP over more than 524 287 items.

Radius search.  hamming_range returns EVERY database item within a Hamming radius of each query (the hash-lookup protocol that
pr_curve's precision-within-radius numbers describe), as a ragged CSR result: offsets int64 [Q+1], and idx / dist / rel of
T = offsets[Q] entries in which query q owns offsets[q]:offsets[q+1], ordered by (distance, database index): bit for bit the first
ball(q) columns of hamming_topk.  `radius` is in calc_hammingDist's units (the dist column); in half-units hr = min(2K,
floor(2 * radius)), and an item belongs to the ball iff h <= hr.  The histogram sizes the lists (the one device-to-host read per
query block is T), cmh_hamming_range fills them: memory is the sum of the balls, not Q x the largest one, and a ball may be wider
than CMH_TOPK_MAX.  Shards fill one allocation in ascending order; empty balls are legal.

Instance-level recall (Recall@K, MedR, mean rank, MRR over PAIRED items: where does the caption of this image rank?).  A rank is a
count: the 0-based position of database item t in the stable ranking of query q is
  #{j : h(q, j) < h(q, t)} + #{j < t : h(q, j) = h(q, t)},
so target_counts makes one walk over the database (cmh_hamming_rank: no list, no sort, any database size, the counts of shards add)
and returns, per (query, target), counts[q, g] = (less, ties_before, ties): items nearer than the target, items as near with a
smaller index, items as near (the target included).  The tie convention is the caller's choice, applied by ranks_from_counts:
  "index"        less + ties_before        the target's column in hamming_topk's row: the module's convention
  "optimistic"   less                      the target first among its ties
  "pessimistic"  less + ties - 1           ... last
  "expected"     less + (ties - 1) / 2     the mean over a uniformly random order of the ties (float64)
recall_from_counts: a query's best rank is the minimum over its targets (-1 in `targets` pads a row), R@K = the share of queries
whose best 1-based rank is <= K, median_rank / mean_rank / mrr over the 1-based best ranks, all over the queries that have a
target.  Under "expected" R@K of a target is clamp((K - less) / ties, 0, 1), the probability that a random tie order puts it in the
first K: exact for one target per query; with several the per-query maximum is taken, a LOWER BOUND of the probability that any
lands there.  MRR has no such closed form and is not defined under "expected".
Bias note: Hamming ties are massive, and under identity pairing t(q) = q the "index" convention favours small q, whose targets
precede most of their ties.  A NumPy check (2000 random 16-bit codes, each query its item with 10 % of the bits flipped: 10 items
on average share the target's distance) gives R@1 = 0.546 over the first half of the queries and 0.399 over the second.  Report
"expected", or both bounds, for paired data."""
import math

import torch

import cmh_native as N

DEFAULT_TOPN = (1,) + tuple(range(50, 1001, 50))
SHARD_ITEMS = N.TOPK_MAX             # database items per shard unless a call says otherwise (tests pass small values)
ITEMS_MAX = 2 ** 31 - 1              # indices and counts are int32
QUERIES_FEW = 64                     # up to this many queries a plain search is ONE cmh_hamming_topk_few over the whole database (_few_route);
                                     # set from the measurement of DESIGN.md 9.6, 0 = nothing routes there


def _dev(*ts):
    for t in ts:
        if t is not None and t.is_cuda:
            return t.device
    if not torch.cuda.is_available():
        raise N.NativeError("utils.retrieval needs a GPU: libcmh has no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _codes(B, dev):
    if B.dim() < 2:
        B = B.unsqueeze(0)
    return N.pack_codes(B.to(dev).float())


def _labels(L, dev):
    return None if L is None else N.pack_labels(L.to(dev).float())


def _cuts(n, step):
    return [(a, min(n, a + step)) for a in range(0, n, step)]


def _rows(t, cut, n):
    """Rows cut[0]:cut[1] of a packed operand of n rows (a tensor, a pair of planes or None): the operand itself when the cut is all
    of it, else views (a row slice of a contiguous row-major tensor is contiguous: nothing is copied)."""
    if t is None or cut == (0, n):
        return t
    if isinstance(t, tuple):
        return tuple(x[cut[0]:cut[1]] for x in t)
    return t[cut[0]:cut[1]]


def _plan(what, qp, rp, shard_items):
    """-> (Q, n, query blocks, database shards) as lists of (begin, end)."""
    Q, n = qp[0].shape[0], rp[0].shape[0]
    step = SHARD_ITEMS if shard_items is None else int(shard_items)
    if not 1 <= step <= N.TOPK_MAX:
        raise N.NativeError(f"{what}: shard_items={step} outside [1, {N.TOPK_MAX}]")
    if n > ITEMS_MAX:
        raise N.NativeError(f"{what}: N={n} exceeds {ITEMS_MAX} (indices and counts are int32)")
    if Q < 1 or n < 1:
        raise N.NativeError(f"{what}: Q={Q} N={n}")
    return Q, n, _cuts(Q, N.QUERIES_MAX), _cuts(n, step)


def _tail(n):
    """The bits of the last mask word that belong to items: all 64 when n is a multiple of 64."""
    r = int(n) % 64
    return -1 if r == 0 else (1 << r) - 1


class ItemMask:
    """One bit per database item: words int64 [ceil(n / 64)], bit j % 64 of word j / 64 set = item j is admitted; n = the items.
    What the constructors and the operators return has zero bits behind n.  from_bool, to_bool, count and & | ~ are plain torch on
    whatever device the words live; from_ids and from_labels run on the GPU (cmh_mask_from_ids / cmh_mask_from_labels)."""

    def __init__(self, words, n):
        n = int(n)
        if n < 1 or n > ITEMS_MAX:
            raise N.NativeError(f"ItemMask: n={n} outside [1, {ITEMS_MAX}]")
        if words.dtype != torch.int64 or words.dim() != 1 or words.numel() != N.mask_words(n):
            raise N.NativeError(f"ItemMask: words are int64 [{N.mask_words(n)}] for n={n}, not {words.dtype} {tuple(words.shape)}")
        self.words, self.n = words.contiguous(), n

    @classmethod
    def all(cls, n, device=None):
        """Every item admitted."""
        words = torch.full((N.mask_words(n),), -1, dtype=torch.int64, device=device)
        words[-1] &= _tail(n)
        return cls(words, n)

    @classmethod
    def from_bool(cls, t):
        """t: [n] booleans (anything whose nonzero entries mean admitted), on any device."""
        t = torch.as_tensor(t)
        if t.dim() != 1 or t.numel() < 1:
            raise N.NativeError(f"ItemMask.from_bool: a tensor [n >= 1], not {tuple(t.shape)}")
        n = t.numel()
        bits = torch.zeros(N.mask_words(n) * 64, dtype=torch.int64, device=t.device)
        bits[:n] = (t != 0).to(torch.int64)
        shifts = torch.arange(64, dtype=torch.int64, device=t.device)
        return cls((bits.view(-1, 64) << shifts).sum(1), n)      # (distinct bits: the sum is their OR; bit 63 is the sign bit)

    @classmethod
    def from_ids(cls, n, ids, keep=True, device=None):
        """keep=True: an allow list (only `ids` admitted); keep=False: a deny list (everything but `ids`).  Duplicates are legal; an
        id outside [0, n) raises."""
        ids = torch.as_tensor(ids)
        if ids.numel() == 0:
            ids = ids.to(torch.int64)                              # (an empty list arrives as float32)
        if ids.is_floating_point() or ids.is_complex() or ids.dtype == torch.bool or ids.dim() > 1:
            raise N.NativeError(f"ItemMask.from_ids: ids are integers [M], not {ids.dtype} {tuple(ids.shape)}")
        dev = _dev(ids) if device is None else torch.device(device)
        ids = ids.reshape(-1).to(dev)
        ids = torch.where((ids < 0) | (ids >= int(n)), torch.full_like(ids, -1), ids)      # (the cast to int32 must not fold a large id into range)
        mask = cls.all(n, dev) if not keep else cls(torch.zeros(N.mask_words(n), dtype=torch.int64, device=dev), n)
        N.mask_from_ids(mask.words, ids.to(torch.int32).contiguous(), n, 1 if keep else 0)      # raises on an id outside [0, n)
        return mask

    @classmethod
    def from_labels(cls, labels, any_of=None, all_of=None, none_of=None, classes=None):
        """labels: multi-hot [n, C] (any dtype but int32) or packed int32 [n, ceil(classes / 32)] (pack_labels; classes = 32 per word
        unless given).  any_of / all_of / none_of: class indices; the item carries at least one of / all of / none of them.  The
        conditions given are ANDed; none given admits everything."""
        if labels is None or labels.dim() != 2 or labels.shape[0] < 1:
            raise N.NativeError("ItemMask.from_labels: labels [n >= 1, C] (multi-hot) or packed int32 [n, LW]")
        dev = _dev(labels)
        if labels.dtype == torch.int32:
            lab = labels.to(dev).contiguous()
            classes = 32 * lab.shape[1] if classes is None else int(classes)
        else:
            lab, classes = _labels(labels, dev), labels.shape[1]
        n, mask = lab.shape[0], None
        for mode, wanted in ((N.MASK_ANY, any_of), (N.MASK_ALL, all_of), (N.MASK_NONE, none_of)):
            if wanted is None:
                continue
            c = torch.as_tensor(wanted, dtype=torch.int64).reshape(-1)
            if c.numel() and (int(c.min()) < 0 or int(c.max()) >= classes):
                raise N.NativeError(f"ItemMask.from_labels: a class outside [0, {classes})")
            hot = torch.zeros(1, classes, dtype=torch.float32)
            hot[0, c] = 1.0
            one = cls(N.mask_from_labels(lab, _labels(hot, dev)[0].contiguous(), mode, classes), n)
            mask = one if mask is None else mask & one
        return cls.all(n, dev) if mask is None else mask

    def to(self, device):
        return ItemMask(self.words.to(device), self.n)

    def to_bool(self):
        """-> bool [n] on the words' device."""
        shifts = torch.arange(64, dtype=torch.int64, device=self.words.device)
        return (((self.words[:, None] >> shifts) & 1) != 0).reshape(-1)[:self.n]

    def count(self):
        """The number of admitted items (a Python int: one read from the device)."""
        return int(self.to_bool().sum())

    def _same(self, other):
        if not isinstance(other, ItemMask) or other.n != self.n:
            raise N.NativeError(f"ItemMask: the operands cover {self.n} and {getattr(other, 'n', other)!r} items")
        return other.words.to(self.words.device)

    def __and__(self, other):
        return ItemMask(self.words & self._same(other), self.n)

    def __or__(self, other):
        return ItemMask(self.words | self._same(other), self.n)

    def __invert__(self):
        words = ~self.words
        words[-1] &= _tail(self.n)
        return ItemMask(words, self.n)


def _check_mask(what, mask, n, bits, k, shard_items=None, graded=False, want_counts=False):
    """What a masked search refuses, by name, before anything touches the GPU: the routes that take no mask and the limits of the
    kernels that do."""
    if not isinstance(mask, ItemMask):
        raise N.NativeError(f"{what}: mask= takes an ItemMask, not {type(mask).__name__}")
    for name, given in (("graded=True", graded), ("want_counts", want_counts), ("shard_items", shard_items is not None)):
        if given:
            raise N.NativeError(f"{what}: {name} and mask= exclude each other (the tiles route takes no mask)")
    if mask.n != n:
        raise N.NativeError(f"{what}: the mask covers {mask.n} items, the database holds {n}")
    if bits > N.FEW_BITS_MAX:
        raise N.NativeError(f"{what}: bits={bits} exceeds {N.FEW_BITS_MAX}, the limit of a masked search")
    if int(k) > N.FEW_K_MAX:
        raise N.NativeError(f"{what}: k={int(k)} exceeds {N.FEW_K_MAX}, the limit of a masked search")
    if not 1 <= int(k) <= n:
        raise N.NativeError(f"{what}: k={int(k)} outside [1, N={n}]")


def _masked_search(what, qp, rp, bits, k, ql, rl, mask):
    """The masked few-query kernel over blocks of FEW_Q_MAX queries -> (idx, dist, rel, found); rel = the hit flags from the gathered
    label words as on the unmasked few route (None without labels), 0 in the pad columns."""
    Q, n = qp[0].shape[0], rp[0].shape[0]
    _check_mask(what, mask, n, bits, k)
    N.check_retrieval_operands(what, qp, rp, bits, ql, rl)
    allow = mask.words.to(rp[0].device)
    parts = [N.hamming_topk_few_masked(_rows(qp, cut, Q), rp, allow, bits, int(k)) for cut in _cuts(Q, N.FEW_Q_MAX)]
    idx, dist, found = parts[0] if len(parts) == 1 else tuple(torch.cat(p) for p in zip(*parts))
    rel = None
    if ql is not None:
        hit = ((rl[idx.clamp(min=0).long()] & ql[:, None, :]) != 0).any(-1)
        rel = (hit & (idx >= 0)).to(torch.uint8)
    return idx, dist, rel, found


def _few_route(Q, k, bits, shard_items, graded, want_counts):
    """Does a search go to the few-query kernel (lanes own items, the whole database in one call) in place of the tiles kernels
    (lanes own queries, shards)?  Decided from what the call shows, never by an option: few queries, a result page of neighbours, a
    code the kernel takes, nothing it does not compute (grades, histograms), and no shard size: a caller who states one is asking
    for shards."""
    return (Q <= min(QUERIES_FEW, N.FEW_Q_MAX) and k <= N.FEW_K_MAX and bits <= N.FEW_BITS_MAX and not graded and not want_counts
            and shard_items is None)


def _search(what, qp, rp, bits, k, ql, rl, shard_items=None, grade_classes=None, want_counts=False):
    """The k nearest database items of every query over any number of shards and query blocks -> (idx, dist, tag, counts): tag =
    hit flags (None without labels), or grades with grade_classes; counts = hamming_hist's, None unless want_counts.
    Per query block: shard 0 is searched with k_0 = min(k, N_0); shard s is searched with min(k, N_s) and folded into the running
    list, whose width is min(k, items so far), through two output buffers of Q x k entries used in turn: O(Q k) memory however
    many shards there are."""
    Q, n, blocks, shards = _plan(what, qp, rp, shard_items)
    k = int(k)
    if not 1 <= k <= n:
        raise N.NativeError(f"{what}: k={k} outside [1, N={n}]")
    if _few_route(Q, k, bits, shard_items, grade_classes is not None, want_counts):
        # the hit flags from the label words of the k results: Q x k x LW integers of glue, equal to the tiles route's flags.  The
        # native call takes no labels, so they are checked here as the tiles route's binding checks them, before anything is gathered
        N.check_retrieval_operands(what, qp, rp, bits, ql, rl)
        idx, dist = N.hamming_topk_few(qp, rp, bits, k)
        rel = None if ql is None else ((rl[idx.long()] & ql[:, None, :]) != 0).any(-1).to(torch.uint8)
        return idx, dist, rel, None

    def one(qcut, scut, kk):
        q, r = _rows(qp, qcut, Q), _rows(rp, scut, n)
        qlab, rlab = _rows(ql, qcut, Q), _rows(rl, scut, n)
        if grade_classes is not None:
            out = N.hamming_topk_graded(q, r, bits, kk, qlab, rlab, want_counts=want_counts, classes=grade_classes)
        else:
            out = N.hamming_topk(q, r, bits, kk, qlab, rlab, want_counts=want_counts)
        return out if want_counts else out + (None,)

    parts = []
    for qcut in blocks:
        idx, dist, tag, counts = one(qcut, shards[0], min(k, shards[0][1]))
        flat = [None, None]
        for s, scut in enumerate(shards[1:]):
            b_idx, b_dist, b_tag, b_counts = one(qcut, scut, min(k, scut[1] - scut[0]))
            idx, dist, tag = _fold((idx, dist, tag), (b_idx, b_dist, b_tag), scut, k, flat, s)
            if want_counts:
                counts = counts + b_counts
        parts.append((idx, dist, tag, counts))
    if len(parts) == 1:
        return parts[0]
    return tuple(None if p[0] is None else torch.cat(p) for p in zip(*parts))


def _fold(run, b, scut, k, flat, s):
    """The running list of the shards before scut and the list b of shard scut -> the running list behind it, min(k, scut[1])
    wide, written into flat[s & 1]: a buffer set of rows x k entries allocated at its first use (two shards never need the second),
    so that step s reads the set step s - 1 wrote and writes the other."""
    rows, w = run[0].shape[0], min(k, scut[1])
    if flat[s & 1] is None:
        flat[s & 1] = tuple(None if t is None else torch.empty(rows * k, dtype=t.dtype, device=t.device) for t in run)
    out = tuple(None if t is None else t[:rows * w].view(rows, w) for t in flat[s & 1])
    return N.topk_merge(run, b, scut[0], w, out=out)


def _summed(what, qp, rp, shard_items, one):
    """one(query cut, shard cut, Q, n) -> an int32 histogram of the block against the shard; summed over the shards (on the GPU),
    concatenated over the query blocks."""
    Q, n, blocks, shards = _plan(what, qp, rp, shard_items)
    parts = []
    for qcut in blocks:
        acc = one(qcut, shards[0], Q, n)
        for scut in shards[1:]:
            acc = acc + one(qcut, scut, Q, n)
        parts.append(acc)
    return parts[0] if len(parts) == 1 else torch.cat(parts)


def _hist(qp, rp, bits, ql, rl, shard_items=None):
    return _summed("pr_curve", qp, rp, shard_items, lambda qc, sc, Q, n: N.hamming_hist(
        _rows(qp, qc, Q), _rows(rp, sc, n), bits, _rows(ql, qc, Q), _rows(rl, sc, n)))


def _grade_hist(ql, rl, classes, shard_items=None):
    return _summed("grade_histogram", (ql,), (rl,), shard_items, lambda qc, sc, Q, n: N.label_overlap_hist(
        _rows(ql, qc, Q), _rows(rl, sc, n), classes))


def _map_count(what, qp, rp, bits, ql, rl, k=None, shard_items=None):
    """mAP by counting over any number of shards and query blocks -> (map 0-dim f32 on the GPU, ap f32 [Q]).  One shard: one
    hamming_ap_partial.  Several: the histogram of the whole database first (the per-shard ones summed), then one call per shard in
    ascending order with the histogram of the shards before it; the float64 sums add in shard order."""
    Q, n, blocks, shards = _plan(what, qp, rp, shard_items)
    if k is not None and int(k) < 1:
        raise N.NativeError(f"{what}: k={k} below 1")
    sums, totals = [], []
    for qcut in blocks:
        q, qlab = _rows(qp, qcut, Q), _rows(ql, qcut, Q)
        if len(shards) == 1:
            acc, total = N.hamming_ap_partial(q, rp, bits, qlab, rl, topk=k, want_counts=True)
        else:
            total = N.hamming_hist(q, _rows(rp, shards[0], n), bits, qlab, _rows(rl, shards[0], n))
            for scut in shards[1:]:
                total = total + N.hamming_hist(q, _rows(rp, scut, n), bits, qlab, _rows(rl, scut, n))
            acc = prior = None
            for scut in shards:
                part, own = N.hamming_ap_partial(q, _rows(rp, scut, n), bits, qlab, _rows(rl, scut, n), topk=k,
                                                 total_counts=total, prior_counts=prior, want_counts=True)
                acc = part if acc is None else acc + part
                prior = own if prior is None else prior + own
        sums.append(acc)
        totals.append(total)
    one = len(sums) == 1
    return N.ap_finish(sums[0] if one else torch.cat(sums), totals[0] if one else torch.cat(totals), bits, topk=k)


def mean_average_precision(qB, rB, query_L, retrieval_L, k=None, shard_items=None, return_ap=False):
    """calc_map_k_matrix with ties by ascending database index (torch.sort(stable=True)), by counting: no ranking, any database up
    to 2^31 - 1 items.  -> mAP as a 0-dim f32 CPU tensor (return_ap: also the per-query APs, f32 [Q] on the GPU).  AP = 0 for a query
    without relevant items; the mean runs over ALL queries in query order, in f32, like the reference's."""
    _classes("mean_average_precision", query_L, retrieval_L)
    dev = _dev(qB, rB)
    mp, ap = _map_count("mean_average_precision", _codes(qB, dev), _codes(rB, dev), rB.shape[1], _labels(query_L, dev),
                        _labels(retrieval_L, dev), k, shard_items)
    mp = mp.cpu()
    return (mp, ap) if return_ap else mp


def radius_half_units(radius, bits):
    """A radius in calc_hammingDist's units -> hr = min(2K, floor(2 * radius)) half-units; negative or NaN is refused."""
    r = float(radius)
    if r != r or r < 0:
        raise N.NativeError(f"radius={radius}: a Hamming radius is a number >= 0")
    return 2 * int(bits) if r >= int(bits) else int(math.floor(2 * r))


def _range(what, qp, rp, bits, hr, ql, rl, shard_items=None, max_hits=None):
    """Every item at half-distance <= hr over any number of shards and query blocks -> (offsets int64 [Q+1], idx int32 [T],
    dist f32 [T], rel uint8 [T] or None without labels).  Per query block: the histogram of the whole database (the per-shard ones
    summed), its balls' prefix sum = the offsets, T read back (the only device-to-host read) and checked against max_hits before
    anything is allocated for the block, one allocation, then one fill per shard in ascending order with the histogram of the
    shards before it.  T = 0 launches no fill."""
    Q, n, blocks, shards = _plan(what, qp, rp, shard_items)
    limit = ITEMS_MAX if max_hits is None else int(max_hits)
    if limit < 0:
        raise N.NativeError(f"{what}: max_hits={max_hits} below 0")
    dev = qp[0].device
    parts, hits = [], 0
    for qcut in blocks:
        q, qlab = _rows(qp, qcut, Q), _rows(ql, qcut, Q)
        total = N.hamming_hist(q, _rows(rp, shards[0], n), bits, qlab, _rows(rl, shards[0], n))
        for scut in shards[1:]:
            total = total + N.hamming_hist(q, _rows(rp, scut, n), bits, qlab, _rows(rl, scut, n))
        off = torch.zeros(qcut[1] - qcut[0] + 1, dtype=torch.int64, device=dev)
        torch.cumsum(total[:, :hr + 1].sum((1, 2)), 0, out=off[1:])
        T = int(off[-1])
        hits += T
        if hits > limit:
            raise N.NativeError(f"{what}: T={hits} hits exceed max_hits={limit}")
        out = (torch.empty(T, dtype=torch.int32, device=dev), torch.empty(T, dtype=torch.float32, device=dev),
               None if ql is None else torch.empty(T, dtype=torch.uint8, device=dev))
        if T:
            row_off, prior = off[:-1], None
            for s, scut in enumerate(shards):
                more = s + 1 < len(shards)
                got = N.hamming_range(q, _rows(rp, scut, n), bits, hr, qlab, _rows(rl, scut, n), total_counts=total, prior_counts=prior,
                                      row_off=row_off, idx_base=scut[0], out=out, want_counts=more)
                if more:
                    prior = got[1] if prior is None else prior + got[1]
        parts.append((off,) + out)
    if len(parts) == 1:
        return parts[0]
    offs, base = [parts[0][0]], parts[0][0][-1]
    for p in parts[1:]:
        offs.append(p[0][1:] + base)
        base = offs[-1][-1]
    return (torch.cat(offs),) + tuple(None if ts[0] is None else torch.cat(ts) for ts in zip(*[p[1:] for p in parts]))


def hamming_range(qB, rB, radius, query_L=None, retrieval_L=None, shard_items=None, max_hits=None):
    """-> (offsets int64 [Q+1], idx int32 [T], dist f32 [T][, rel uint8 [T] with labels]) on the GPU: every database code within
    `radius` (calc_hammingDist's units) of every query; query q's list is idx[offsets[q]:offsets[q+1]], ordered by (distance,
    database index).  T = offsets[Q]; more than max_hits (default 2^31 - 1) entries are refused before they are allocated."""
    if (query_L is None) != (retrieval_L is None):
        raise N.NativeError("hamming_range: labels on one side only")
    hr = radius_half_units(radius, rB.shape[-1])
    dev = _dev(qB, rB)
    off, idx, dist, rel = _range("hamming_range", _codes(qB, dev), _codes(rB, dev), rB.shape[-1], hr, _labels(query_L, dev),
                                 _labels(retrieval_L, dev), shard_items, max_hits)
    return (off, idx, dist) if rel is None else (off, idx, dist, rel)


def hamming_topk(qB, rB, k, query_L=None, retrieval_L=None, shard_items=None, mask=None):
    """-> (idx int32 [Q, k], dist f32 [Q, k][, rel uint8 [Q, k] with labels]): the k nearest database codes of every query.
    mask=ItemMask: among the items it admits -> (idx, dist, rel or None, found int32 [Q]); pads idx = -1, dist = +inf, rel = 0."""
    if (query_L is None) != (retrieval_L is None):
        raise N.NativeError("hamming_topk: labels on one side only")
    if mask is not None:
        _check_mask("hamming_topk", mask, rB.shape[0], rB.shape[1], k, shard_items)
        dev = _dev(qB, rB)
        return _masked_search("hamming_topk", _codes(qB, dev), _codes(rB, dev), rB.shape[1], k, _labels(query_L, dev),
                              _labels(retrieval_L, dev), mask)
    dev = _dev(qB, rB)
    idx, dist, rel, _ = _search("hamming_topk", _codes(qB, dev), _codes(rB, dev), rB.shape[1], k, _labels(query_L, dev),
                                _labels(retrieval_L, dev), shard_items)
    return (idx, dist) if rel is None else (idx, dist, rel)


def _soft_search(what, u, rp, bits, k, mask=None):
    """-> (idx int32 [Q, k], dist f32 [Q, k], wdist int32 [Q, k]) of soft queries u f32 [Q, bits] against packed planes: blocks of
    SOFT_Q_MAX queries, one cmh_soft_topk each over the whole database.  mask=ItemMask: cmh_soft_topk_masked, and found int32 [Q]
    as a fourth element; the pad columns hold idx = -1, dist = +inf, wdist = 2^31 - 1."""
    if u.dim() < 2:
        u = u.unsqueeze(0)
    n, k = rp[0].shape[0], int(k)
    if mask is not None:
        _check_mask(what, mask, n, bits, k)
    if u.shape[1] != bits:
        raise N.NativeError(f"{what}: {u.shape[1]}-entry soft queries for codes of {bits} bits")
    if bits > N.SOFT_BITS_MAX:
        raise N.NativeError(f"{what}: bits={bits} exceeds {N.SOFT_BITS_MAX}, the limit of the soft search (no other route computes its distance)")
    if k > N.SOFT_K_MAX:
        raise N.NativeError(f"{what}: k={k} exceeds {N.SOFT_K_MAX}, the limit of the soft search (no other route computes its distance)")
    if not 1 <= k <= n:
        raise N.NativeError(f"{what}: k={k} outside [1, N={n}]")
    if u.shape[0] < 1 or n > ITEMS_MAX:
        raise N.NativeError(f"{what}: Q={u.shape[0]} N={n}")
    qs, qm, _, scale = N.soft_query_planes(u.to(rp[0].device).float())
    unit = scale / torch.full_like(scale, 30.0)      # (tensor / tensor: one IEEE division; by a Python number the GPU multiplies by 1 / 30)
    if mask is not None:
        allow = mask.words.to(rp[0].device)
        parts = [N.soft_topk_masked((qs[a:b], qm[a:b]), rp, allow, bits, k) for a, b in _cuts(u.shape[0], N.SOFT_Q_MAX)]
        idx, wdist, found = parts[0] if len(parts) == 1 else tuple(torch.cat(p) for p in zip(*parts))
        dist = wdist.float() * unit[:, None]
        return idx, torch.where(idx >= 0, dist, torch.full_like(dist, float("inf"))), wdist, found
    parts = [N.soft_topk((qs[a:b], qm[a:b]), rp, bits, k) for a, b in _cuts(u.shape[0], N.SOFT_Q_MAX)]
    idx, wdist = parts[0] if len(parts) == 1 else tuple(torch.cat(p) for p in zip(*parts))
    return idx, wdist.float() * unit[:, None], wdist


def _soft_rel(out, ql, rl):
    """A soft search's tuple with the hit flags of its idx appended: rel uint8 [Q, k] gathered from the label words of the k results
    as _search's few route gathers them; 0 in the pad columns (idx = -1) of a masked search."""
    idx = out[0]
    rel = ((rl[idx.clamp(min=0).long()] & ql[:, None, :]) != 0).any(-1) & (idx >= 0)
    return out + (rel.to(torch.uint8),)


def _check_soft(what, u, bits, query_L, retrieval_L, both=False):
    """What a soft call refuses by name before anything touches the GPU -> u as [Q, bits]."""
    if u.dim() < 2:
        u = u.unsqueeze(0)
    if (query_L is None) != (retrieval_L is None):
        raise N.NativeError(f"{what}: labels on one side only")
    if both and query_L is None:
        raise N.NativeError(f"{what}: needs the labels of both sides")
    if u.shape[1] != bits:
        raise N.NativeError(f"{what}: {u.shape[1]}-entry soft queries for codes of {bits} bits")
    if bits > N.SOFT_BITS_MAX:
        raise N.NativeError(f"{what}: bits={bits} exceeds {N.SOFT_BITS_MAX}, the limit of the soft search (no other route computes its distance)")
    if query_L is not None and query_L.shape[0] != u.shape[0]:
        raise N.NativeError(f"{what}: labels of {query_L.shape[0]} queries for {u.shape[0]} soft queries")
    if not u.is_cuda and not bool(torch.isfinite(u).all()):
        raise N.NativeError(f"{what}: a soft query must be finite (NaN or Inf in the head's output)")
    return u


def soft_topk(u, rB, k, mask=None, query_L=None, retrieval_L=None):
    """-> (idx int32 [Q, k], dist f32 [Q, k], wdist int32 [Q, k]): the k nearest database codes rB (f32 in {-1, 0, +1}) of every
    soft query u (f32 [Q, K], the head's output before its code rule), by (wdist, database index); dist = wdist * (max|u| / 30).
    mask=ItemMask: among the items it admits -> (idx, dist, wdist, found int32 [Q]).  With the labels of both sides rel uint8 [Q, k]
    (the result shares a label with the query; 0 in pad columns) is appended as the last element."""
    if query_L is not None or retrieval_L is not None:
        u = _check_soft("soft_topk", u, rB.shape[-1], query_L, retrieval_L)
    if mask is not None:
        _check_mask("soft_topk", mask, rB.shape[0], rB.shape[-1], k)
    dev = _dev(u, rB)
    out = _soft_search("soft_topk", u, _codes(rB, dev), rB.shape[-1], k, mask)
    return out if query_L is None else _soft_rel(out, _labels(query_L, dev), _labels(retrieval_L, dev))


def _soft_map(what, u, rp, bits, ql, rl, k=None):
    """mAP of soft queries by counting over any number of queries -> (map 0-dim f32 on the GPU, ap f32 [Q], relevant int32 [Q],
    rank_sum int64 [Q]): blocks of SOFT_Q_MAX queries, one cmh_soft_ap each over the whole database; ONE f32 mean over all the
    queries in query order (cmh_map_mean)."""
    n = rp[0].shape[0]
    if k is not None and not 1 <= int(k) <= n:
        raise N.NativeError(f"{what}: k={k} outside [1, N={n}]")
    if u.shape[0] < 1 or n > ITEMS_MAX:
        raise N.NativeError(f"{what}: Q={u.shape[0]} N={n}")
    q = N.soft_query_planes(u.to(rp[0].device).float())
    parts = [N.soft_ap((q[0][a:b], q[1][a:b]), rp, bits, ql[a:b], rl, k) for a, b in _cuts(u.shape[0], N.SOFT_Q_MAX)]
    ap, relevant, rank_sum = parts[0] if len(parts) == 1 else tuple(torch.cat(p) for p in zip(*parts))
    return N.map_mean(ap), ap, relevant, rank_sum


def soft_mean_average_precision(u, rB, query_L, retrieval_L, k=None, return_ap=False):
    """mean_average_precision for soft queries u (f32 [Q, K], the head's output before its code rule): the mAP over the first k
    (None: all) database codes in ascending (wdist, database index), by counting: no ranking, any number of queries, any database up
    to 2^31 - 1 items.  -> mAP as a 0-dim f32 CPU tensor; return_ap: (mAP, ap f32 [Q], relevant int32 [Q], rank_sum int64 [Q]) with
    the three on the GPU: relevant = the query's relevant items, rank_sum = the sum of their ranks (auc_from_rank_sum)."""
    u = _check_soft("soft_mean_average_precision", u, rB.shape[-1], query_L, retrieval_L, both=True)
    dev = _dev(u, rB)
    mp, ap, relevant, rank_sum = _soft_map("soft_mean_average_precision", u, _codes(rB, dev), rB.shape[-1], _labels(query_L, dev),
                                           _labels(retrieval_L, dev), k)
    mp = mp.cpu()
    return (mp, ap, relevant, rank_sum) if return_ap else mp


def auc_from_rank_sum(rank_sum, relevant, n):
    """Per-query ROC-AUC from the rank sums of the relevant items (ties broken by database index like the ranks): U = rank_sum -
    R (R + 1) / 2 pairs (relevant, other) are in the wrong order; AUC = 1 - U / (R (n - R)).  Integers in Python / int64, one float64
    division -> float64 CPU tensor [Q]; NaN where R = 0 or R = n."""
    s = torch.as_tensor(rank_sum).detach().cpu().to(torch.int64).reshape(-1)
    r = torch.as_tensor(relevant).detach().cpu().to(torch.int64).reshape(-1)
    n = int(n)
    if s.numel() != r.numel():
        raise ValueError(f"auc_from_rank_sum: {s.numel()} rank sums for {r.numel()} relevant counts")
    out = torch.full((s.numel(),), float("nan"), dtype=torch.float64)
    for i, (si, ri) in enumerate(zip(s.tolist(), r.tolist())):
        if not 0 <= ri <= n or (ri and not ri * (ri + 1) // 2 <= si <= ri * (ri + 1) // 2 + ri * (n - ri)):
            raise ValueError(f"auc_from_rank_sum: rank_sum={si} is not the rank sum of R={ri} among n={n} items")
        if 0 < ri < n:
            out[i] = 1.0 - (si - ri * (ri + 1) // 2) / (ri * (n - ri))
    return out


def soft_topn_precision(u, rB, query_L, retrieval_L, topn=DEFAULT_TOPN):
    """topn_precision for soft queries -> (precision [len(topn)], recall [len(topn)], rel uint8 [Q, max(topn)] on the GPU) of the
    soft ranking's first N items; max(topn) <= SOFT_K_MAX.  The recall's denominators are cmh_soft_ap's relevant counts."""
    u = _check_soft("soft_topn_precision", u, rB.shape[-1], query_L, retrieval_L, both=True)
    topn = [int(t) for t in topn]
    dev = _dev(u, rB)
    rp, ql, rl = _codes(rB, dev), _labels(query_L, dev), _labels(retrieval_L, dev)
    rel = _soft_rel(_soft_search("soft_topn_precision", u, rp, rB.shape[-1], max(topn)), ql, rl)[-1]
    relevant = _soft_map("soft_topn_precision", u, rp, rB.shape[-1], ql, rl)[2]
    precision, recall = topn_from_rel(rel, relevant, topn)
    return precision, recall, rel


def _classes(what, query_L, retrieval_L):
    if query_L is None or retrieval_L is None:
        raise N.NativeError(f"{what}: needs the labels of both sides")
    if query_L.dim() != 2 or retrieval_L.dim() != 2 or query_L.shape[1] != retrieval_L.shape[1]:
        raise N.NativeError(f"{what}: labels of shapes {tuple(query_L.shape)} and {tuple(retrieval_L.shape)}")
    return query_L.shape[1]


def graded_topk(qB, rB, k, query_L, retrieval_L, shard_items=None):
    """-> (idx int32 [Q, k], dist f32 [Q, k], grade uint8 [Q, k]): hamming_topk's neighbours with the number of labels each shares
    with its query where hamming_topk has the hit flag (rel == grade > 0).  At most 255 classes."""
    classes = _classes("graded_topk", query_L, retrieval_L)
    dev = _dev(qB, rB)
    return _search("graded_topk", _codes(qB, dev), _codes(rB, dev), rB.shape[1], k, _labels(query_L, dev), _labels(retrieval_L, dev),
                   shard_items, grade_classes=classes)[:3]


def grade_histogram(query_L, retrieval_L, shard_items=None):
    """-> int32 [Q, C+1] on the GPU: entry [q, g] = database items that share exactly g labels with query q."""
    classes = _classes("grade_histogram", query_L, retrieval_L)
    dev = _dev(query_L, retrieval_L)
    return _grade_hist(_labels(query_L, dev), _labels(retrieval_L, dev), classes, shard_items)


def graded_from_grades(grade, grade_counts, topn):
    """grade [Q, k] = grades of the ranking's first k columns, grade_counts [Q, C+1] = database items per grade, topn <= k ->
    (ndcg [len(topn)], acg [len(topn)], wap [len(topn)]) float64 CPU tensors.  IDCG@n comes from the histogram: the ideal ranking
    holds the grades in descending order, so grade v fills the positions behind those of all higher grades, and its share is
    (2^v - 1) * (D[end] - D[start]) with D the prefix sum of 1 / log2(i + 1) and both ends cut at n."""
    g = grade.detach().cpu().to(torch.int64)
    c = grade_counts.detach().cpu().to(torch.int64)
    topn = [int(n) for n in topn]
    if not topn or min(topn) < 1 or max(topn) > g.shape[1]:
        raise ValueError(f"topn {topn} outside [1, {g.shape[1]}]")
    if c.dim() != 2 or c.shape[0] != g.shape[0]:
        raise ValueError(f"grade_counts of shape {tuple(c.shape)} for {g.shape[0]} queries")
    keep = c[:, 1:].sum(1) > 0
    if not bool(keep.any()):
        z = torch.zeros(len(topn), dtype=torch.float64)
        return z, z.clone(), z.clone()
    g, c = g[keep], c[keep]
    cols = [n - 1 for n in topn]
    k = g.shape[1]
    pos = torch.arange(1, k + 1, dtype=torch.float64)
    disc = 1.0 / torch.log2(pos + 1.0)
    acg = g.cumsum(1).double() / pos                                  # ACG@i for every i <= k
    hit = g > 0
    hits = hit.cumsum(1).double()
    wap = torch.where(hits > 0, (acg * hit).cumsum(1) / hits.clamp(min=1), torch.zeros_like(acg))
    dcg = ((torch.exp2(g.double()) - 1.0) * disc).cumsum(1)[:, cols]
    D = torch.cat([torch.zeros(1, dtype=torch.float64), disc.cumsum(0)])
    down = c[:, 1:].flip(1)                                           # counts of the grades C, C-1, ..., 1
    gain = torch.exp2(torch.arange(c.shape[1] - 1, 0, -1, dtype=torch.float64)) - 1.0
    end = down.cumsum(1)
    start = end - down
    idcg = torch.stack([((D[end.clamp(max=n)] - D[start.clamp(max=n)]) * gain).sum(1) for n in topn], 1)
    return (dcg / idcg).mean(0), acg[:, cols].mean(0), wap[:, cols].mean(0)


def graded_metrics(qB, rB, query_L, retrieval_L, topn=DEFAULT_TOPN, grade_counts=None, shard_items=None):
    """-> (ndcg [len(topn)], acg [len(topn)], wap [len(topn)], grade uint8 [Q, max(topn)] on the GPU).  grade_counts: a
    grade_histogram of the same labels, to share it among the directions of an evaluation (computed here when None)."""
    topn = [int(n) for n in topn]
    _, _, grade = graded_topk(qB, rB, max(topn), query_L, retrieval_L, shard_items)
    if grade_counts is None:
        grade_counts = grade_histogram(query_L, retrieval_L, shard_items)
    return graded_from_grades(grade, grade_counts, topn) + (grade,)


def curves_from_counts(counts):
    """counts [Q, H, 2] integers (hamming_hist) -> (precision [H], recall [H]) float64 CPU tensors; entry h = the ball of
    half-distance <= h, i.e. calc_hammingDist <= h / 2."""
    c = counts.detach().cpu().to(torch.int64)
    hits = c[:, :, 1].cumsum(1)
    ball = c.sum(2).cumsum(1)
    relevant = hits[:, -1]
    keep = relevant > 0
    H = c.shape[1]
    if not bool(keep.any()):
        return torch.zeros(H, dtype=torch.float64), torch.zeros(H, dtype=torch.float64)
    hits, ball, relevant = hits[keep].double(), ball[keep].double(), relevant[keep].double()
    precision = torch.where(ball > 0, hits / ball.clamp(min=1), torch.zeros_like(hits))
    return precision.mean(0), (hits / relevant[:, None]).mean(0)


def topn_from_rel(rel, relevant, topn):
    """rel [Q, k] hit flags of the ranking's first k columns, relevant [Q] = relevant items in the database, topn <= k ->
    (precision [len(topn)], recall [len(topn)]) float64 CPU tensors."""
    r = rel.detach().cpu().to(torch.int64)
    relevant = relevant.detach().cpu().to(torch.int64)
    topn = [int(n) for n in topn]
    if not topn or min(topn) < 1 or max(topn) > r.shape[1]:
        raise ValueError(f"topn {topn} outside [1, {r.shape[1]}]")
    keep = relevant > 0
    if not bool(keep.any()):
        z = torch.zeros(len(topn), dtype=torch.float64)
        return z, z.clone()
    hits = r[keep].cumsum(1)[:, [n - 1 for n in topn]].double()
    n = torch.tensor(topn, dtype=torch.float64)
    return (hits / n).mean(0), (hits / relevant[keep].double()[:, None]).mean(0)


def pr_curve(qB, rB, query_L, retrieval_L, shard_items=None):
    """-> (precision [2K+1], recall [2K+1], counts int32 [Q, 2K+1, 2] on the GPU).  Entry h is the Hamming ball of radius h / 2
    (codes without zeros only reach the even entries; entry 2r is then the usual P@H<=r)."""
    dev = _dev(qB, rB)
    counts = _hist(_codes(qB, dev), _codes(rB, dev), rB.shape[1], _labels(query_L, dev), _labels(retrieval_L, dev), shard_items)
    precision, recall = curves_from_counts(counts)
    return precision, recall, counts


def topn_precision(qB, rB, query_L, retrieval_L, topn=DEFAULT_TOPN, shard_items=None):
    """-> (precision [len(topn)], recall [len(topn)], rel uint8 [Q, max(topn)] on the GPU) of the ranking's first N items."""
    dev = _dev(qB, rB)
    topn = [int(n) for n in topn]
    qp, rp = _codes(qB, dev), _codes(rB, dev)
    ql, rl = _labels(query_L, dev), _labels(retrieval_L, dev)
    _, _, rel, counts = _search("topn_precision", qp, rp, rB.shape[1], max(topn), ql, rl, shard_items, want_counts=True)
    relevant = counts[:, :, 1].sum(1)
    precision, recall = topn_from_rel(rel, relevant, topn)
    return precision, recall, rel


RANK_TIES = ("index", "optimistic", "pessimistic", "expected")
RECALL_KS = (1, 5, 10)


def _targets(what, targets, Q, n, dev):
    """targets: integers [Q] or [Q, G], database indices, -1 = padding -> int64 [Q, G] on dev; anything else is refused."""
    t = torch.as_tensor(targets)
    if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise N.NativeError(f"{what}: targets are integer database indices, not {t.dtype}")
    if t.dim() == 1:
        t = t[:, None]
    if t.dim() != 2 or t.shape[0] != Q or t.shape[1] < 1:
        raise N.NativeError(f"{what}: targets of shape {tuple(t.shape)} for {Q} queries ([Q] or [Q, G])")
    t = t.to(dev).long()
    if bool(((t < -1) | (t >= n)).any()):
        raise N.NativeError(f"{what}: a target outside 0..{n - 1} (-1 pads a row)")
    return t


def _target_counts(what, qp, rp, bits, targets, shard_items=None):
    """(less, ties_before, ties) of every (query, target) over any number of shards, query blocks and blocks of RANK_TARGETS_MAX
    targets -> int64 [Q, G, 3].  The targets' planes are rows of the packed database (index_select); for the shard [a, b) the bound
    is clamp(t - a, 0, b - a): all of a shard behind the target, none of one before it; the shards' counts add."""
    Q, n, blocks, shards = _plan(what, qp, rp, shard_items)
    t = _targets(what, targets, Q, n, qp[0].device)
    parts = []
    for qcut in blocks:
        q, cols = _rows(qp, qcut, Q), []
        for g0 in range(0, t.shape[1], N.RANK_TARGETS_MAX):
            tt = t[qcut[0]:qcut[1], g0:g0 + N.RANK_TARGETS_MAX]
            rows = tt.clamp(min=0).reshape(-1)
            tp = tuple(x.index_select(0, rows) for x in rp)
            acc = None
            for a, b in shards:
                bound = torch.where(tt >= 0, (tt - a).clamp(0, b - a), tt).to(torch.int32).contiguous()
                c = N.hamming_rank(q, _rows(rp, (a, b), n), bits, tp, bound).long()
                acc = c if acc is None else acc + c
            cols.append(acc)
        parts.append(cols[0] if len(cols) == 1 else torch.cat(cols, 1))
    return parts[0] if len(parts) == 1 else torch.cat(parts)


def target_counts(qB, rB, targets, shard_items=None):
    """-> int64 [Q, G, 3] on the GPU: (less, ties_before, ties) of database item targets[q, g] in the ranking of query q (see the
    module docstring); a padding slot (-1) gives three zeros.  targets: integers [Q] or [Q, G]."""
    dev = _dev(qB, rB)
    return _target_counts("target_counts", _codes(qB, dev), _codes(rB, dev), rB.shape[-1], targets, shard_items)


def _counts3(counts):
    c = counts.detach().cpu().to(torch.int64)
    if c.dim() != 3 or c.shape[2] != 3:
        raise ValueError(f"counts of shape {tuple(c.shape)}: [Q, G, 3] of target_counts")
    return c[:, :, 0], c[:, :, 1], c[:, :, 2]


def _tie_rule(ties):
    if ties not in RANK_TIES:
        raise ValueError(f"ties={ties!r}: one of {RANK_TIES}")
    return ties


def ranks_from_counts(counts, ties="index"):
    """counts [Q, G, 3] (target_counts) -> the 0-based rank of every target under the tie convention: int64 [Q, G] on the CPU, -1
    for padding ("expected": float64, NaN for padding)."""
    less, before, tied = _counts3(counts)
    ties = _tie_rule(ties)
    pad = tied == 0                                                    # a target is one of its own ties
    if ties == "expected":
        r = less.double() + (tied - 1).double() / 2
        return torch.where(pad, torch.full_like(r, float("nan")), r)
    r = less + before if ties == "index" else less if ties == "optimistic" else less + tied - 1
    return torch.where(pad, torch.full_like(r, -1), r)


class _Metrics(dict):
    """recall_from_counts' result; under ties="expected" it has no "mrr", and asking for it says why."""

    def __missing__(self, key):
        if key == "mrr":
            raise N.NativeError('recall_from_counts: mrr is not defined under ties="expected" (no closed form over random tie orders)')
        raise KeyError(key)


def recall_from_counts(counts, ks=RECALL_KS, ties="index"):
    """counts [Q, G, 3] (target_counts, on any device) -> {"recall": float64 [len(ks)], "median_rank", "mean_rank", "mrr": floats
    over the 1-based best ranks, "best_rank": [Q] 1-based, -1 without a target ("expected": float64, NaN)}; float64 arithmetic on
    the CPU.  Means run over the queries with at least one target (all zeros when there is none).  "expected": see the module
    docstring; no "mrr"."""
    less, _, tied = _counts3(counts)
    ties = _tie_rule(ties)
    ks = [int(k) for k in ks]
    if not ks or min(ks) < 1:
        raise ValueError(f"ks {ks}: cut-offs >= 1")
    r = ranks_from_counts(counts, ties)
    pad = tied == 0
    has = ~pad.all(1)
    expected = ties == "expected"
    if expected:
        best = torch.where(pad, torch.full_like(r, float("inf")), r).min(1).values + 1.0
        best = torch.where(has, best, torch.full_like(best, float("nan")))
        hit = [((k - less).double() / tied.clamp(min=1).double()).clamp(0, 1).masked_fill(pad, 0.0).max(1).values for k in ks]
    else:
        best = torch.where(pad, torch.full_like(r, torch.iinfo(torch.int64).max - 1), r).min(1).values + 1
        best = torch.where(has, best, torch.full_like(best, -1))
        hit = [(best <= k).double() for k in ks]
    out = _Metrics(best_rank=best)
    if not bool(has.any()):
        out.update(recall=torch.zeros(len(ks), dtype=torch.float64), median_rank=0.0, mean_rank=0.0)
        if not expected:
            out["mrr"] = 0.0
        return out
    b = best[has].double()
    s = b.sort().values
    out.update(recall=torch.stack([h[has].mean() for h in hit]), median_rank=float((s[(s.numel() - 1) // 2] + s[s.numel() // 2]) / 2),
               mean_rank=float(b.mean()))
    if not expected:
        out["mrr"] = float((1.0 / b).mean())
    return out


def _identity(what, Q, n):
    if Q > n:
        raise N.NativeError(f"{what}: identity pairing needs Q={Q} <= N={n} (pass targets)")
    return torch.arange(Q)


def recall_at_k(qB, rB, targets=None, ks=RECALL_KS, ties="index", shard_items=None):
    """Recall@K, MedR, mean rank and MRR of paired items: recall_from_counts of target_counts, plus "counts" (int64 [Q, G, 3] on
    the GPU) for any other convention.  targets=None: identity pairing t(q) = q, the paired test-set protocol (Q <= N)."""
    _tie_rule(ties)
    dev = _dev(qB, rB)
    qp, rp = _codes(qB, dev), _codes(rB, dev)
    if targets is None:
        targets = _identity("recall_at_k", qp[0].shape[0], rp[0].shape[0])
    counts = _target_counts("recall_at_k", qp, rp, rB.shape[-1], targets, shard_items)
    out = recall_from_counts(counts, ks, ties)
    out["counts"] = counts
    return out


def _nz_mask(bits, dev):
    """int32 [W]: the nz words of a code without zeros - every word full, the last one up to `bits`."""
    mask = torch.full(((bits + 31) // 32,), -1, dtype=torch.int32, device=dev)
    if bits % 32:
        mask[-1] = (1 << (bits % 32)) - 1
    return mask


def _no_zeros(what, whose, planes, bits):
    """The table's keys are sign words: a code with a 0 entry (a cleared nz bit inside `bits`) has no key and is refused."""
    mask = _nz_mask(bits, planes[1].device)
    if not bool(((planes[1] & mask) == mask).all()):
        raise N.NativeError(f"{what}: {whose} with a 0 entry: the bucket table holds codes in {{-1, +1}} only (hamming_range / "
                            "range_search take codes with zeros)")


def _check_lookup(what, bits, query_bits, radius):
    """What a lookup refuses by name before anything is packed, built or launched."""
    if query_bits != bits:
        raise N.NativeError(f"{what}: {query_bits}-bit queries for an index of {bits} bits")
    if bits > N.BUCKET_BITS_MAX:
        raise N.NativeError(f"{what}: {bits}-bit codes exceed BUCKET_BITS_MAX = {N.BUCKET_BITS_MAX} (range_search takes them)")
    if isinstance(radius, bool) or radius != int(radius) or not 0 <= int(radius) <= N.BUCKET_RADIUS_MAX:
        raise N.NativeError(f"{what}: radius={radius} is not a whole number of bits in [0, BUCKET_RADIUS_MAX = {N.BUCKET_RADIUS_MAX}] "
                            "(range_search takes any radius)")


class BucketTable:
    """The items of a packed database grouped by equal code (csrc/retrieval_buckets.hip), all on the GPU:
      order  int32 [n]      the item indices sorted by key (the sign words cut to `bits`, word W - 1 most significant), equal keys
                            by ascending index
      starts int32 [U + 1]  bucket b = order[starts[b]:starts[b + 1]]
      codes  int32 [U, W]   the key of each bucket, ascending
      bits, n, n_buckets (= U)
    build(planes, bits) sorts once (cmh_code_sort, cmh_code_bucket_count / _fill; U is the one number read back);
    lookup(...) answers "the items whose code is the query's with at most `radius` bits flipped" at a cost that does not grow
    with n.  Codes in {-1, +1} only."""

    def __init__(self, order, starts, codes, bits, n):
        self.order, self.starts, self.codes, self.bits, self.n, self.n_buckets = order, starts, codes, int(bits), int(n), codes.shape[0]

    @classmethod
    def build(cls, planes, bits):
        """planes: (sign, nz) of pack_codes, int32 [n, ceil(bits / 32)] on the GPU, any n up to 2^31 - 1."""
        bits = int(bits)
        sign, nz = planes
        N.fit("BucketTable.build", (nz, tuple(sign.shape)))
        _no_zeros("BucketTable.build", "a database code", planes, bits)
        sign = sign.contiguous()
        order = N.code_sort(sign, bits)
        starts, codes = N.code_buckets(sign, order, bits)
        return cls(order, starts, codes, bits, sign.shape[0])

    def counts(self):
        """int32 [U]: the items of each bucket."""
        return self.starts[1:] - self.starts[:-1]

    def lookup(self, query_codes, radius=0, query_labels=None, retrieval_L=None):
        """-> hamming_range's tuple (offsets int64 [Q+1], idx int32 [T], dist f32 [T][, rel uint8 [T] with labels]): every item
        within `radius` (0, 1 or 2 whole bits) of every query, by (distance, database index) inside a query's list.  query_codes
        f32 [Q, bits] in {-1, +1}; query_labels / retrieval_L: multi-hot [Q, C] / [n, C], both or neither."""
        if (query_labels is None) != (retrieval_L is None):
            raise N.NativeError("BucketTable.lookup: labels on one side only")
        if retrieval_L is not None and retrieval_L.shape[0] != self.n:
            raise N.NativeError(f"BucketTable.lookup: labels of {retrieval_L.shape[0]} items for a table of {self.n}")
        _check_lookup("BucketTable.lookup", self.bits, query_codes.shape[-1], radius)
        dev = self.order.device
        return self._lookup("BucketTable.lookup", _codes(query_codes, dev), radius, _labels(query_labels, dev), _labels(retrieval_L, dev))

    def _lookup(self, what, qp, radius, ql, rl):
        """The packed form: qp = the queries' planes, ql / rl = packed labels or None -> (offsets, idx, dist, rel or None).  Per block
        of queries: count pass, cumsum, the two totals read back, fill pass, the hit buckets expanded to items through `order`,
        and for radius >= 1 one stable sort on (query, distance, item)."""
        radius = int(radius)
        _no_zeros(what, "a query", qp, self.bits)
        dev = self.order.device
        Q = qp[0].shape[0]
        parts = []
        for cut in _cuts(Q, N.QUERIES_MAX):
            qs = _rows(qp[0], cut, Q).contiguous()
            nq = cut[1] - cut[0]
            n_buckets, n_items = N.bucket_probe_count(qs, self.codes, self.starts, self.bits, radius)
            boff = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
            torch.cumsum(n_buckets, 0, out=boff[1:])
            off = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
            torch.cumsum(n_items, 0, out=off[1:])
            TB, T = torch.stack((boff[-1], off[-1])).tolist()
            if T > ITEMS_MAX:
                raise N.NativeError(f"{what}: T={T} hits exceed {ITEMS_MAX}")
            if TB == 0:
                idx, dist = torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.float32, device=dev)
                query = torch.empty(0, dtype=torch.int64, device=dev)
            else:
                bucket, bdist = N.bucket_probe_fill(qs, self.codes, self.starts, self.bits, radius, boff, TB)
                bucket = bucket.long()
                first = self.starts[bucket].long()
                size = self.starts[bucket + 1].long() - first
                hit = torch.repeat_interleave(torch.arange(TB, device=dev), size, output_size=T)      # the hit each item came from
                begin = torch.cumsum(size, 0) - size
                idx = self.order[first[hit] + (torch.arange(T, device=dev) - begin[hit])]
                dist = bdist[hit]
                query = torch.repeat_interleave(torch.arange(nq, device=dev), n_buckets.long(), output_size=TB)[hit]
                if radius >= 1:      # a distance level is many buckets: merge them by index (radius 0: one bucket, already ascending)
                    by = torch.sort(((query * (N.BUCKET_RADIUS_MAX + 1) + dist) << 31) + idx, stable=True)[1]
                    idx, dist, query = idx[by], dist[by], query[by]
                dist = dist.to(torch.float32)
            rel = None if ql is None else ((_rows(ql, cut, Q)[query] & rl[idx.long()]) != 0).any(-1).to(torch.uint8)
            parts.append((off, idx, dist, rel))
        if len(parts) == 1:
            return parts[0]
        offs, base = [parts[0][0]], parts[0][0][-1]
        for p in parts[1:]:
            offs.append(p[0][1:] + base)
            base = offs[-1][-1]
        return (torch.cat(offs),) + tuple(None if ts[0] is None else torch.cat(ts) for ts in zip(*[p[1:] for p in parts]))


def substring_radii(bits, radius):
    """The radius each 16-bit substring of a `bits`-bit code is probed at for a whole-bit search radius (multi-index hashing,
    csrc/retrieval_mih.hip): with m = ceil(bits / 16) and a, b = divmod(radius, m), a_j = a for j <= b and a - 1 behind; -1 = the
    substring is not probed.  If every probed j had d_j > a_j, then d >= (b + 1)(a + 1) + (m - b - 1) a = m a + b + 1 > radius, so
    an item within the radius is within a_j of the query in some probed substring.  a <= MIH_SUB_RADIUS_MAX: radius <= 3 m - 1."""
    if isinstance(bits, bool) or bits != int(bits) or not 1 <= int(bits) <= N.BUCKET_BITS_MAX:
        raise N.NativeError(f"substring_radii: {bits}-bit codes outside [1, BUCKET_BITS_MAX = {N.BUCKET_BITS_MAX}] (range_search takes them)")
    m = N.mih_substrings(bits)
    top = (N.MIH_SUB_RADIUS_MAX + 1) * m - 1
    if isinstance(radius, bool) or radius != int(radius) or not 0 <= int(radius) <= top:
        raise N.NativeError(f"substring_radii: radius={radius} is not a whole number of bits in [0, {top}] for {int(bits)}-bit codes "
                            f"({m} substrings, each probed within {N.MIH_SUB_RADIUS_MAX}; range_search takes any radius)")
    a, b = divmod(int(radius), m)
    return [a if j <= b else a - 1 for j in range(m)]


def knn_steps(bits, r_cap):
    """The growth steps 0 .. r_cap of the k-nearest search through the substring tables (csrc/retrieval_mih.hip) ->
    [(substring, level)]: with m = ceil(bits / 16), step s = t m + j (t = 0, 1, 2; j < m) probes substring j at EXACTLY level t,
    the keys that are the query's with exactly t of the substring's bits flipped.  After steps 0 .. r substring j has been probed
    at every level up to substring_radii(bits, r)[j], so every item within r whole bits has been reached; item x is first reached
    at step min_j (d_j m + j), a unique minimum (the j are distinct below m), and counts there alone.  r_cap <= 3 m - 1."""
    try:
        m = len(substring_radii(bits, r_cap))
    except N.NativeError as e:
        raise N.NativeError(f"knn_steps: {e}".replace("radius=", "r_cap=")) from None
    return [(s % m, s // m) for s in range(int(r_cap) + 1)]


MAX_BALL_SHARE = 64                  # SubstringTables.topk answers a query through the tables while its ball is at most 1 / 64 of the
                                     # database: set from the measurement of DESIGN.md 9.13 (level with the scan at about 2 %, behind at 5 %)
MAX_HITS_TOPK = 2 ** 28              # entries of one fill of SubstringTables.topk: 2 GiB of idx + dist.  A memory budget, not a measurement


def _check_far(what, bits, query_bits, radius):
    """What a substring lookup refuses by name before anything is packed, built or launched."""
    if query_bits != bits:
        raise N.NativeError(f"{what}: {query_bits}-bit queries for an index of {bits} bits")
    try:
        substring_radii(bits, radius)
    except N.NativeError as e:
        raise N.NativeError(f"{what}: {e}") from None


def _check_topk(what, bits, n, query_bits, k, r_cap, max_ball, max_hits):
    """What a k-nearest search through the substring tables refuses by name before anything is packed, built or launched ->
    (r_cap, max_ball, max_hits) with the defaults in: r_cap = 3 ceil(bits / 16) - 1, max_ball = n // MAX_BALL_SHARE, max_hits =
    MAX_HITS_TOPK."""
    if query_bits != bits:
        raise N.NativeError(f"{what}: {query_bits}-bit queries for an index of {bits} bits")
    if bits > N.BUCKET_BITS_MAX:
        raise N.NativeError(f"{what}: {bits}-bit codes exceed BUCKET_BITS_MAX = {N.BUCKET_BITS_MAX} (search takes them)")
    if isinstance(k, bool) or k != int(k) or not 1 <= int(k) <= n:
        raise N.NativeError(f"{what}: k={k} outside [1, N={n}]")
    top = (N.MIH_SUB_RADIUS_MAX + 1) * N.mih_substrings(bits) - 1
    r_cap = top if r_cap is None else r_cap
    if isinstance(r_cap, bool) or r_cap != int(r_cap) or not 0 <= int(r_cap) <= top:
        raise N.NativeError(f"{what}: r_cap={r_cap} is not a whole number of bits in [0, {top}] for {bits}-bit codes")
    max_ball = n // MAX_BALL_SHARE if max_ball is None else int(max_ball)
    max_hits = MAX_HITS_TOPK if max_hits is None else int(max_hits)
    if max_ball < 0 or max_hits < 0:
        raise N.NativeError(f"{what}: max_ball={max_ball}, max_hits={max_hits}: below 0")
    return int(r_cap), max_ball, max_hits


class SubstringTables:
    """Multi-index hashing over a packed database (csrc/retrieval_mih.hip), all on the GPU: one direct-addressed
    table per 16-bit substring of the codes.
      order  int32 [m, n]       row j = the item indices by ascending (key of substring j, index)
      starts int32 [m, 65537]   bucket `key` of table j = order[j, starts[j, key]:starts[j, key + 1]]
      sign   int32 [n, W]       the database's sign plane (candidates are verified against it)
      bits, n, m (= ceil(bits / 16)), max_radius (= 3 m - 1)
    build(planes, bits) sorts m times (cmh_mih_build); lookup(...) answers "every item within `radius` whole bits" by probing each
    table at substring_radii(bits, radius) and verifying the buckets' items: the cost follows the buckets' sizes, not n;
    topk(...) answers "the k nearest items" by growing every query's radius (knn_steps; cmh_mih_knn_count / _fill).  Codes in
    {-1, +1} only, up to 128 bit."""

    def __init__(self, order, starts, sign, bits, n):
        self.order, self.starts, self.sign, self.bits, self.n, self.m = order, starts, sign, int(bits), int(n), order.shape[0]
        self._nz = None                                            # the scan route's nz plane: _planes() makes it on first use

    @property
    def max_radius(self):
        return (N.MIH_SUB_RADIUS_MAX + 1) * self.m - 1

    @classmethod
    def build(cls, planes, bits):
        """planes: (sign, nz) of pack_codes, int32 [n, ceil(bits / 32)] on the GPU, any n up to 2^31 - 1."""
        bits = int(bits)
        sign, nz = planes
        N.fit("SubstringTables.build", (nz, tuple(sign.shape)))
        if bits > N.BUCKET_BITS_MAX:
            raise N.NativeError(f"SubstringTables.build: {bits}-bit codes exceed BUCKET_BITS_MAX = {N.BUCKET_BITS_MAX} (range_search takes them)")
        _no_zeros("SubstringTables.build", "a database code", planes, bits)
        sign = sign.contiguous()
        order, starts = N.mih_build(sign, bits)
        return cls(order, starts, sign, bits, sign.shape[0])

    def lookup(self, query_codes, radius, query_labels=None, retrieval_L=None, max_hits=None):
        """-> hamming_range's tuple (offsets int64 [Q+1], idx int32 [T], dist f32 [T][, rel uint8 [T] with labels]): every item
        within `radius` whole bits (0 .. max_radius) of every query, by (distance, database index) inside a query's list.
        query_codes f32 [Q, bits] in {-1, +1}; query_labels / retrieval_L: multi-hot [Q, C] / [n, C], both or neither; more than
        max_hits (default 2^31 - 1) entries are refused before they are allocated."""
        if (query_labels is None) != (retrieval_L is None):
            raise N.NativeError("SubstringTables.lookup: labels on one side only")
        if retrieval_L is not None and retrieval_L.shape[0] != self.n:
            raise N.NativeError(f"SubstringTables.lookup: labels of {retrieval_L.shape[0]} items for tables of {self.n}")
        _check_far("SubstringTables.lookup", self.bits, query_codes.shape[-1], radius)
        dev = self.order.device
        off, idx, dist, rel = self._lookup("SubstringTables.lookup", _codes(query_codes, dev), radius, _labels(query_labels, dev),
                                           _labels(retrieval_L, dev), max_hits)
        return (off, idx, dist) if rel is None else (off, idx, dist, rel)

    def _lookup(self, what, qp, radius, ql, rl, max_hits=None):
        """The packed form: qp = the queries' planes, ql / rl = packed labels or None -> (offsets, idx, dist, rel or None).  Per block
        of queries: count pass, cumsum, the total read back and checked, fill pass, one stable sort on (query, distance, item)."""
        radius = int(radius)
        _no_zeros(what, "a query", qp, self.bits)
        limit = ITEMS_MAX if max_hits is None else int(max_hits)
        if limit < 0:
            raise N.NativeError(f"{what}: max_hits={max_hits} below 0")
        dev = self.order.device
        Q = qp[0].shape[0]
        parts, hits = [], 0
        for cut in _cuts(Q, N.QUERIES_MAX):
            qs = _rows(qp[0], cut, Q).contiguous()
            nq = cut[1] - cut[0]
            n_hits = N.mih_count(qs, self.sign, self.bits, radius, self.order, self.starts)
            off = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
            torch.cumsum(n_hits, 0, out=off[1:])
            T = int(off[-1])
            hits += T
            if hits > limit:
                raise N.NativeError(f"{what}: T={hits} hits exceed max_hits={limit}")
            if T == 0:
                idx, dist = torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.float32, device=dev)
                query = torch.empty(0, dtype=torch.int64, device=dev)
            else:
                idx, dist = N.mih_fill(qs, self.sign, self.bits, radius, self.order, self.starts, off, T)
                query = torch.repeat_interleave(torch.arange(nq, device=dev), n_hits.long(), output_size=T)
                by = torch.sort(((query * (self.bits + 1) + dist) << 31) + idx, stable=True)[1]      # the walk's order -> (distance, item)
                idx, dist = idx[by], dist[by].to(torch.float32)
            rel = None if ql is None else ((_rows(ql, cut, Q)[query] & rl[idx.long()]) != 0).any(-1).to(torch.uint8)
            parts.append((off, idx, dist, rel))
        if len(parts) == 1:
            return parts[0]
        offs, base = [parts[0][0]], parts[0][0][-1]
        for p in parts[1:]:
            offs.append(p[0][1:] + base)
            base = offs[-1][-1]
        return (torch.cat(offs),) + tuple(None if ts[0] is None else torch.cat(ts) for ts in zip(*[p[1:] for p in parts]))

    def topk(self, query_codes, k, query_labels=None, retrieval_L=None, r_cap=None, max_ball=None, max_hits=None):
        """-> hamming_topk's tuple (idx int32 [Q, k], dist f32 [Q, k][, rel uint8 [Q, k] with labels]), bit for bit: the k nearest
        items of every query, distance ascending, ties by database index, found by growing each query's radius through the tables
        (knn_steps) until its ball holds k items: the cost follows that ball, not n.  A query whose ball within r_cap (default
        max_radius) holds fewer than k items, or whose ball holds more than max_ball (default n // MAX_BALL_SHARE) items, is
        answered by the scan instead; max_hits (default MAX_HITS_TOPK) bounds the entries of one fill, and a ball beyond it goes
        to the scan too.
        query_codes f32 [Q, bits] in {-1, +1}; query_labels / retrieval_L: multi-hot [Q, C] / [n, C], both or neither."""
        if (query_labels is None) != (retrieval_L is None):
            raise N.NativeError("SubstringTables.topk: labels on one side only")
        if retrieval_L is not None and retrieval_L.shape[0] != self.n:
            raise N.NativeError(f"SubstringTables.topk: labels of {retrieval_L.shape[0]} items for tables of {self.n}")
        caps = _check_topk("SubstringTables.topk", self.bits, self.n, query_codes.shape[-1], k, r_cap, max_ball, max_hits)
        dev = self.order.device
        idx, dist, rel = self._topk("SubstringTables.topk", _codes(query_codes, dev), k, _labels(query_labels, dev),
                                    _labels(retrieval_L, dev), *caps)
        return (idx, dist) if rel is None else (idx, dist, rel)

    def _planes(self):
        """(sign, nz) of the database for the scan route: the codes hold no 0, so nz is _nz_mask in every row (made on first use)."""
        if self._nz is None:
            self._nz = _nz_mask(self.bits, self.sign.device).repeat(self.n, 1).contiguous()
        return self.sign, self._nz

    def _topk(self, what, qp, k, ql, rl, r_cap, max_ball, max_hits, shard_items=None):
        """The packed form -> (idx, dist, rel or None).  Per block of queries: the count pass (r*, |ball(r*)| per query), ONE host read
        of both, then the admitted queries (r* >= 0, ball within max_ball and max_hits) in groups of consecutive queries whose balls
        sum to at most max_hits: cumsum, fill, one stable sort on (query, distance, item), the first k of every list gathered; the
        other queries go through _search (the scan) as gathered rows and are scattered back."""
        k = int(k)
        _no_zeros(what, "a query", qp, self.bits)
        dev = self.order.device
        Q = qp[0].shape[0]
        out_idx = torch.empty(Q, k, dtype=torch.int32, device=dev)
        out_dist = torch.empty(Q, k, dtype=torch.float32, device=dev)
        for cut in _cuts(Q, N.QUERIES_MAX):
            qs = _rows(qp[0], cut, Q).contiguous()
            nq = cut[1] - cut[0]
            radius, n_ball, _ = N.mih_knn_count(qs, self.sign, self.bits, k, r_cap, self.order, self.starts)
            admitted = (radius >= 0) & (n_ball <= min(max_ball, max_hits))
            walk = torch.where(admitted, radius, torch.full_like(radius, -1))
            sizes = torch.where(admitted, n_ball, torch.zeros_like(n_ball)).long()
            ends = torch.cumsum(sizes, 0)
            host_admitted, host_ends = torch.stack((admitted.long(), ends)).cpu()        # the block's one read (two small vectors)
            begin = 0
            while begin < nq:                                                          # groups of consecutive queries within max_hits
                base = int(host_ends[begin - 1]) if begin else 0
                end = max(begin + 1, int(torch.searchsorted(host_ends, base + max_hits, right=True)))
                T = int(host_ends[end - 1]) - base
                if T:
                    off = torch.zeros(end - begin + 1, dtype=torch.int64, device=dev)
                    off[1:] = ends[begin:end] - base
                    idx, dist = N.mih_knn_fill(qs[begin:end], self.sign, self.bits, walk[begin:end].contiguous(), self.order,
                                               self.starts, off, T)
                    query = torch.repeat_interleave(torch.arange(end - begin, device=dev), sizes[begin:end], output_size=T)
                    by = torch.sort(((query * (self.bits + 1) + dist) << 31) + idx, stable=True)[1]   # the walk's order -> (distance, item)
                    rows = torch.nonzero(admitted[begin:end]).squeeze(1)                # an admitted ball holds at least k items
                    first = by[(off[rows][:, None] + torch.arange(k, device=dev)[None, :]).reshape(-1)]
                    out_idx[cut[0] + begin + rows] = idx[first].view(-1, k)
                    out_dist[cut[0] + begin + rows] = dist[first].view(-1, k).to(torch.float32)
                begin = end
            if not bool(host_admitted.all()):
                rows = torch.nonzero(~admitted).squeeze(1) + cut[0]
                scan = _search(what, tuple(p[rows] for p in qp), self._planes(), self.bits, k, None, None, shard_items)
                out_idx[rows], out_dist[rows] = scan[0], scan[1]
        rel = None if ql is None else ((rl[out_idx.long()] & ql[:, None, :]) != 0).any(-1).to(torch.uint8)
        return out_idx, out_dist, rel


class CodeIndex:
    """A database of hash codes, packed once.  search(query_codes, k) -> hamming_topk's tuple (graded=True: graded_topk's);
    buckets() -> the BucketTable of the index (built on first use, dropped by add()); lookup(query_codes, radius) -> the radius
    search of range_search through that table (radius 0, 1, 2; codes without zeros); bucket_stats() -> how the items spread over
    their distinct codes; substrings() -> the SubstringTables of the index (likewise built on first use), lookup_far(query_codes,
    radius) -> range_search's tuple through them for a whole-bit radius up to 3 ceil(bits / 16) - 1, near_duplicates(radius) ->
    duplicates' tuple through them, search_tables(query_codes, k) -> search's tuple through them (the radius grown per query);
    search_soft(u, k) -> soft_topk's; map_soft(u, query_labels) -> soft_mean_average_precision's; mask(...) -> an ItemMask for search(..., mask=) / search_soft(..., mask=);
    range_search(query_codes, radius) -> hamming_range's; duplicates(radius) -> the index's near-duplicate lists;
    rank_of(query_codes, targets) -> target_counts'; recall(query_codes, targets) -> recall_at_k's; stats() -> code_stats'.
    Any size up to 2^31 - 1 items: the search runs over shards of `shard_items` rows (None: SHARD_ITEMS), views of ONE buffer per
    plane that add() grows geometrically, so many small add()s never make many small shards.  save() / load() keep the packed
    planes and labels as one .npz (data only)."""

    def __init__(self, codes, labels=None, shard_items=None):
        dev = _dev(codes)
        self.bits = codes.shape[1]
        self.size = 0
        self.classes = None if labels is None else labels.shape[1]
        self.device = dev
        self.shard_items = shard_items
        self._sign = self._nz = self._lab = None
        self._append(_codes(codes, dev), _labels(labels, dev))

    @property
    def planes(self):
        """(sign, nz) int32 [size, ceil(bits / 32)]: views of the buffers' filled rows."""
        return self._sign[:self.size], self._nz[:self.size]

    @property
    def labels(self):
        return None if self._lab is None else self._lab[:self.size]

    def _append(self, planes, lab):
        new = planes[0].shape[0]
        if self.size + new > ITEMS_MAX:
            raise N.NativeError(f"CodeIndex: {self.size} + {new} items exceed {ITEMS_MAX} (indices are int32)")

        def grown(buf, rows):
            if buf is not None and self.size + new <= buf.shape[0]:
                buf[self.size:self.size + new] = rows
                return buf
            cap = self.size + new if buf is None else min(ITEMS_MAX, max(self.size + new, 2 * buf.shape[0]))
            out = torch.empty(cap, rows.shape[1], dtype=rows.dtype, device=rows.device)
            if self.size:
                out[:self.size] = buf[:self.size]
            out[self.size:self.size + new] = rows
            return out

        self._sign, self._nz = grown(self._sign, planes[0]), grown(self._nz, planes[1])
        if lab is not None:
            self._lab = grown(self._lab, lab)
        self.size += new
        self._buckets = self._substrings = None                    # derived from the items: buckets() / substrings() build them again

    def add(self, codes, labels=None):
        """Appends items behind the ones the index holds (their indices: size, size + 1, ...); only the new rows are packed."""
        if codes.dim() < 2:
            codes = codes.unsqueeze(0)
        if codes.shape[1] != self.bits:
            raise N.NativeError(f"CodeIndex.add: {codes.shape[1]}-bit codes for an index of {self.bits} bits")
        if (labels is None) != (self.classes is None):
            raise N.NativeError("CodeIndex.add: labels given for an index without them" if self.classes is None
                                else "CodeIndex.add: the index holds labels, the new items bring none")
        if labels is not None and (labels.dim() != 2 or labels.shape[1] != self.classes or labels.shape[0] != codes.shape[0]):
            raise N.NativeError(f"CodeIndex.add: labels of shape {tuple(labels.shape)} for {codes.shape[0]} items of {self.classes} classes")
        if codes.shape[0]:
            self._append(_codes(codes, self.device), _labels(labels, self.device))
        return self

    def save(self, path):
        """The packed planes, the packed labels (when there are any), bits, classes and size as one .npz: arrays only."""
        import numpy as np
        arrays = {"sign": self.planes[0].cpu().numpy(), "nz": self.planes[1].cpu().numpy(), "bits": np.int64(self.bits),
                  "size": np.int64(self.size), "classes": np.int64(0 if self.classes is None else self.classes)}
        if self._lab is not None:
            arrays["labels"] = self.labels.cpu().numpy()
        with open(path, "wb") as f:
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path, shard_items=None):
        """An index written by save(); nothing is packed again."""
        import numpy as np
        with np.load(path, allow_pickle=False) as z:
            bits, size, classes = int(z["bits"]), int(z["size"]), int(z["classes"])
            sign, nz = torch.from_numpy(z["sign"]), torch.from_numpy(z["nz"])
            lab = torch.from_numpy(z["labels"]) if "labels" in z.files else None
        W = (bits + 31) // 32
        ok = bits >= 1 and size >= 1 and tuple(sign.shape) == (size, W) and tuple(nz.shape) == (size, W) and sign.dtype == torch.int32 \
            and nz.dtype == torch.int32 and (classes > 0) == (lab is not None)
        if ok and lab is not None:
            ok = tuple(lab.shape) == (size, (classes + 31) // 32) and lab.dtype == torch.int32
        if not ok:
            raise N.NativeError(f"CodeIndex.load: {path} is not a file written by CodeIndex.save")
        self = cls.__new__(cls)
        self.device = _dev()
        self.bits, self.size, self.classes, self.shard_items = bits, 0, (classes if classes > 0 else None), shard_items
        self._sign = self._nz = self._lab = None
        self._append((sign.to(self.device), nz.to(self.device)), None if lab is None else lab.to(self.device))
        return self

    @classmethod
    def from_mat(cls, path, side="r_img"):
        """The database side ("r_img" | "r_txt") of a file written by TrainBase.save_mat, with its labels r_l."""
        if side not in ("r_img", "r_txt"):
            raise ValueError(f"side {side!r}: r_img or r_txt")
        import scipy.io as scio
        m = scio.loadmat(path)
        labels = torch.from_numpy(m["r_l"]).float() if "r_l" in m else None
        return cls(torch.from_numpy(m[side]).float(), labels)

    def map(self, query_codes, query_labels, k=None, return_ap=False):
        """mean_average_precision of the queries against the index (which must hold labels)."""
        if self.labels is None:
            raise N.NativeError("CodeIndex.map: the index holds no labels")
        if query_labels is None or query_labels.dim() != 2 or query_labels.shape[1] != self.classes:
            raise N.NativeError(f"CodeIndex.map: needs query labels of {self.classes} classes")
        qp = _codes(query_codes, self.device)
        if query_codes.shape[-1] != self.bits:
            raise N.NativeError(f"CodeIndex.map: {query_codes.shape[-1]}-bit queries for an index of {self.bits} bits")
        mp, ap = _map_count("CodeIndex.map", qp, self.planes, self.bits, _labels(query_labels, self.device), self.labels, k,
                            self.shard_items)
        mp = mp.cpu()
        return (mp, ap) if return_ap else mp

    def mask(self, any_of=None, all_of=None, none_of=None, ids=None, exclude_ids=None):
        """An ItemMask over the index's items as they are NOW (after add() it no longer fits and is refused): the items that carry at
        least one class of any_of, all of all_of and none of none_of (the index must hold labels), that are among `ids` and not
        among `exclude_ids`.  The conditions given are ANDed; none given admits everything."""
        if (any_of is not None or all_of is not None or none_of is not None) and self.labels is None:
            raise N.NativeError("CodeIndex.mask: a label condition (any_of / all_of / none_of) on an index without labels")
        m = ItemMask.all(self.size, self.device) if self.labels is None else \
            ItemMask.from_labels(self.labels, any_of, all_of, none_of, classes=self.classes)
        if ids is not None:
            m = m & ItemMask.from_ids(self.size, ids, keep=True, device=self.device)
        if exclude_ids is not None:
            m = m & ItemMask.from_ids(self.size, exclude_ids, keep=False, device=self.device)
        return m

    def search(self, query_codes, k, query_labels=None, graded=False, mask=None):
        """mask=ItemMask (CodeIndex.mask): among the items it admits -> (idx, dist, rel or None, found)."""
        if query_labels is not None and self.labels is None:
            raise N.NativeError("CodeIndex.search: query labels given, but the index has none")
        if mask is not None:
            _check_mask("CodeIndex.search", mask, self.size, self.bits, k, self.shard_items, graded)
        ql = _labels(query_labels, self.device)
        rl = self.labels if ql is not None else None
        if mask is not None:
            return _masked_search("CodeIndex.search", _codes(query_codes, self.device), self.planes, self.bits, k, ql, rl, mask)
        if graded:
            if ql is None:
                raise N.NativeError("CodeIndex.search: graded=True needs query labels and an index with labels")
            return _search("CodeIndex.search", _codes(query_codes, self.device), self.planes, self.bits, k, ql, rl, self.shard_items,
                           grade_classes=self.classes)[:3]
        idx, dist, rel, _ = _search("CodeIndex.search", _codes(query_codes, self.device), self.planes, self.bits, k, ql, rl,
                                    self.shard_items)
        return (idx, dist) if rel is None else (idx, dist, rel)

    def search_soft(self, u, k, mask=None, query_labels=None):
        """soft_topk of the soft queries u (f32 [Q, bits], QueryEncoder.encode_*(..., soft=True)) against the index: (idx, dist,
        wdist).  Any number of queries; bits <= 128 and k <= 4096.  mask=ItemMask: (idx, dist, wdist, found).  query_labels (the
        index must hold labels): rel uint8 [Q, k] is appended as the last element."""
        if u.shape[-1] != self.bits:
            raise N.NativeError(f"CodeIndex.search_soft: {u.shape[-1]}-entry soft queries for an index of {self.bits} bits")
        if query_labels is not None:
            if self.labels is None:
                raise N.NativeError("CodeIndex.search_soft: query labels given, but the index has none")
            if query_labels.dim() != 2 or query_labels.shape[1] != self.classes:
                raise N.NativeError(f"CodeIndex.search_soft: needs query labels of {self.classes} classes")
            u = _check_soft("CodeIndex.search_soft", u, self.bits, query_labels, query_labels)
        out = _soft_search("CodeIndex.search_soft", u, self.planes, self.bits, k, mask)
        return out if query_labels is None else _soft_rel(out, _labels(query_labels, self.device), self.labels)

    def map_soft(self, u, query_labels, k=None, return_ap=False):
        """soft_mean_average_precision of the soft queries u against the index (which must hold labels)."""
        if self.labels is None:
            raise N.NativeError("CodeIndex.map_soft: the index holds no labels")
        if query_labels is None or query_labels.dim() != 2 or query_labels.shape[1] != self.classes:
            raise N.NativeError(f"CodeIndex.map_soft: needs query labels of {self.classes} classes")
        u = _check_soft("CodeIndex.map_soft", u, self.bits, query_labels, query_labels, both=True)
        mp, ap, relevant, rank_sum = _soft_map("CodeIndex.map_soft", u, self.planes, self.bits, _labels(query_labels, self.device),
                                               self.labels, k)
        mp = mp.cpu()
        return (mp, ap, relevant, rank_sum) if return_ap else mp

    def range_search(self, query_codes, radius, query_labels=None, max_hits=None):
        """hamming_range of the queries against the index: (offsets, idx, dist[, rel with query labels])."""
        if query_labels is not None and self.labels is None:
            raise N.NativeError("CodeIndex.range_search: query labels given, but the index has none")
        if query_codes.shape[-1] != self.bits:
            raise N.NativeError(f"CodeIndex.range_search: {query_codes.shape[-1]}-bit queries for an index of {self.bits} bits")
        ql = _labels(query_labels, self.device)
        off, idx, dist, rel = _range("CodeIndex.range_search", _codes(query_codes, self.device), self.planes, self.bits,
                                     radius_half_units(radius, self.bits), ql, self.labels if ql is not None else None,
                                     self.shard_items, max_hits)
        return (off, idx, dist) if rel is None else (off, idx, dist, rel)

    def buckets(self):
        """The BucketTable of the index as it is now: built on first use and kept until add() changes the items.  Derived data:
        save() does not store it.  An index with a code that holds a 0 is refused."""
        if self._buckets is None:
            self._buckets = BucketTable.build(self.planes, self.bits)
        return self._buckets

    def lookup(self, query_codes, radius=0, query_labels=None):
        """range_search(query_codes, radius) through the bucket table: the same tuple, element for element, for radius 0, 1 or 2
        whole bits, codes up to 128 bit and no 0 entry on either side; at a cost that does not grow with the index."""
        if query_labels is not None and self.labels is None:
            raise N.NativeError("CodeIndex.lookup: query labels given, but the index has none")
        _check_lookup("CodeIndex.lookup", self.bits, query_codes.shape[-1], radius)
        ql = _labels(query_labels, self.device)
        off, idx, dist, rel = self.buckets()._lookup("CodeIndex.lookup", _codes(query_codes, self.device), radius, ql,
                                                     self.labels if ql is not None else None)
        return (off, idx, dist) if rel is None else (off, idx, dist, rel)

    def substrings(self):
        """The SubstringTables of the index as it is now: built on first use and kept until add() changes the items.  Derived data:
        save() does not store them.  An index with a code that holds a 0, or of more than 128 bits, is refused."""
        if self._substrings is None:
            self._substrings = SubstringTables.build(self.planes, self.bits)
        return self._substrings

    def search_tables(self, query_codes, k, query_labels=None, **caps):
        """search(query_codes, k) through the substring tables (SubstringTables.topk; caps: r_cap, max_ball, max_hits): the same
        tuple, bit for bit, for codes up to 128 bit and no 0 entry on either side; the cost follows the size of the k-th
        neighbour's Hamming ball, not the size of the index (DESIGN.md 9.13 says when that wins).  Nothing routes here by itself."""
        if query_labels is not None and self.labels is None:
            raise N.NativeError("CodeIndex.search_tables: query labels given, but the index has none")
        unknown = set(caps) - {"r_cap", "max_ball", "max_hits"}
        if unknown:
            raise TypeError(f"CodeIndex.search_tables: unknown option {sorted(unknown)[0]!r} (r_cap, max_ball, max_hits)")
        limits = _check_topk("CodeIndex.search_tables", self.bits, self.size, query_codes.shape[-1], k, caps.get("r_cap"),
                             caps.get("max_ball"), caps.get("max_hits"))
        tables = self.substrings()
        ql = _labels(query_labels, self.device)
        idx, dist, rel = tables._topk("CodeIndex.search_tables", _codes(query_codes, self.device), k, ql,
                                      self.labels if ql is not None else None, *limits, shard_items=self.shard_items)
        return (idx, dist) if rel is None else (idx, dist, rel)

    def lookup_far(self, query_codes, radius, query_labels=None, max_hits=None):
        """range_search(query_codes, radius) through the substring tables: the same tuple, element for element, for a whole-bit
        radius up to 3 ceil(bits / 16) - 1 (11 at 64 bit, 23 at 128), codes up to 128 bit and no 0 entry on either side; the
        cost follows the sizes of the probed buckets, not the size of the index (DESIGN.md 9.12 says when that wins)."""
        if query_labels is not None and self.labels is None:
            raise N.NativeError("CodeIndex.lookup_far: query labels given, but the index has none")
        _check_far("CodeIndex.lookup_far", self.bits, query_codes.shape[-1], radius)
        ql = _labels(query_labels, self.device)
        off, idx, dist, rel = self.substrings()._lookup("CodeIndex.lookup_far", _codes(query_codes, self.device), radius, ql,
                                                        self.labels if ql is not None else None, max_hits)
        return (off, idx, dist) if rel is None else (off, idx, dist, rel)

    def bucket_stats(self):
        """How the items spread over their distinct codes (utils/code_stats.py::bucket_stats_from_sizes): distinct, singletons,
        largest, collisions, collision_probability, bucket_entropy_bits, used_share and the (size, buckets) occupancy table.  Only
        the table of distinct bucket sizes comes to the host."""
        from utils.code_stats import bucket_stats_from_sizes
        sizes, size_counts = torch.unique(self.buckets().counts(), return_counts=True)
        return bucket_stats_from_sizes(self.size, sizes.cpu(), size_counts.cpu(), bits=self.bits)

    def rank_of(self, query_codes, targets):
        """target_counts of the queries against the index: int64 [Q, G, 3] = (less, ties_before, ties) of item targets[q, g]."""
        if query_codes.shape[-1] != self.bits:
            raise N.NativeError(f"CodeIndex.rank_of: {query_codes.shape[-1]}-bit queries for an index of {self.bits} bits")
        return _target_counts("CodeIndex.rank_of", _codes(query_codes, self.device), self.planes, self.bits, targets, self.shard_items)

    def recall(self, query_codes, targets=None, ks=RECALL_KS, ties="index"):
        """recall_at_k of the queries against the index (targets=None: query q belongs to item q)."""
        _tie_rule(ties)
        if targets is None:
            targets = _identity("CodeIndex.recall", query_codes.shape[0] if query_codes.dim() > 1 else 1, self.size)
        counts = self.rank_of(query_codes, targets)
        out = recall_from_counts(counts, ks, ties)
        out["counts"] = counts
        return out

    def stats(self, paired=None):
        """The code diagnostics of the index (utils/code_stats.py: bit balance, dead and duplicated bits, bit correlations; with
        labels in the index the class / bit tables) -> code_stats' dict.  paired: the other modality's codes of the same items (a
        CodeIndex, codes or planes): adds the per-bit agreement and the cross-correlation."""
        from utils.code_stats import code_stats
        return code_stats(self, paired=paired)

    def duplicates(self, radius=0, max_hits=None):
        """The index searched against itself: for every item the OTHER items within `radius`, as hamming_range's CSR tuple (rel when
        the index holds labels).  An item's own entry is taken out of its list (it is there whenever the item lies within the
        radius of itself: a code with z zeros is at distance z / 2 from itself).  max_hits bounds the lists before that."""
        off, idx, dist, rel = _range("CodeIndex.duplicates", self.planes, self.planes, self.bits, radius_half_units(radius, self.bits),
                                     self.labels, self.labels, self.shard_items, max_hits)
        return self._without_own(off, idx, dist, rel)

    def near_duplicates(self, radius, max_hits=None):
        """duplicates(radius), element for element, through the substring tables: the index looked up against itself in blocks of
        queries, an item's own entry taken out.  The limits are lookup_far's."""
        _check_far("CodeIndex.near_duplicates", self.bits, self.bits, radius)
        off, idx, dist, rel = self.substrings()._lookup("CodeIndex.near_duplicates", self.planes, radius, self.labels, self.labels, max_hits)
        return self._without_own(off, idx, dist, rel)

    def _without_own(self, off, idx, dist, rel):
        """The lists of the index against itself without each item's own entry."""
        ball = off[1:] - off[:-1]
        item = torch.repeat_interleave(torch.arange(self.size, device=self.device), ball, output_size=idx.numel())
        keep = idx != item
        own = torch.zeros(self.size, dtype=torch.int64, device=self.device).index_add_(0, item, (~keep).to(torch.int64))
        out = torch.zeros_like(off)
        torch.cumsum(ball - own, 0, out=out[1:])
        return (out, idx[keep], dist[keep]) + (() if rel is None else (rel[keep],))
