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
on the labels only: one call serves all directions of an evaluation) and is what IDCG is computed from, without sorting anything."""
import torch

import cmh_native as N

DEFAULT_TOPN = (1,) + tuple(range(50, 1001, 50))


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


def hamming_topk(qB, rB, k, query_L=None, retrieval_L=None):
    """-> (idx int32 [Q, k], dist f32 [Q, k][, rel uint8 [Q, k] with labels]): the k nearest database codes of every query."""
    if (query_L is None) != (retrieval_L is None):
        raise N.NativeError("hamming_topk: labels on one side only")
    dev = _dev(qB, rB)
    idx, dist, rel = N.hamming_topk(_codes(qB, dev), _codes(rB, dev), rB.shape[1], k, _labels(query_L, dev), _labels(retrieval_L, dev))
    return (idx, dist) if rel is None else (idx, dist, rel)


def _classes(what, query_L, retrieval_L):
    if query_L is None or retrieval_L is None:
        raise N.NativeError(f"{what}: needs the labels of both sides")
    if query_L.dim() != 2 or retrieval_L.dim() != 2 or query_L.shape[1] != retrieval_L.shape[1]:
        raise N.NativeError(f"{what}: labels of shapes {tuple(query_L.shape)} and {tuple(retrieval_L.shape)}")
    return query_L.shape[1]


def graded_topk(qB, rB, k, query_L, retrieval_L):
    """-> (idx int32 [Q, k], dist f32 [Q, k], grade uint8 [Q, k]): hamming_topk's neighbours with the number of labels each shares
    with its query where hamming_topk has the hit flag (rel == grade > 0).  At most 255 classes."""
    classes = _classes("graded_topk", query_L, retrieval_L)
    dev = _dev(qB, rB)
    return N.hamming_topk_graded(_codes(qB, dev), _codes(rB, dev), rB.shape[1], k, _labels(query_L, dev), _labels(retrieval_L, dev),
                                 classes=classes)


def grade_histogram(query_L, retrieval_L):
    """-> int32 [Q, C+1] on the GPU: entry [q, g] = database items that share exactly g labels with query q."""
    classes = _classes("grade_histogram", query_L, retrieval_L)
    dev = _dev(query_L, retrieval_L)
    return N.label_overlap_hist(_labels(query_L, dev), _labels(retrieval_L, dev), classes)


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


def graded_metrics(qB, rB, query_L, retrieval_L, topn=DEFAULT_TOPN, grade_counts=None):
    """-> (ndcg [len(topn)], acg [len(topn)], wap [len(topn)], grade uint8 [Q, max(topn)] on the GPU).  grade_counts: a
    grade_histogram of the same labels, to share it among the directions of an evaluation (computed here when None)."""
    topn = [int(n) for n in topn]
    _, _, grade = graded_topk(qB, rB, max(topn), query_L, retrieval_L)
    if grade_counts is None:
        grade_counts = grade_histogram(query_L, retrieval_L)
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


def pr_curve(qB, rB, query_L, retrieval_L):
    """-> (precision [2K+1], recall [2K+1], counts int32 [Q, 2K+1, 2] on the GPU).  Entry h is the Hamming ball of radius h / 2
    (codes without zeros only reach the even entries; entry 2r is then the usual P@H<=r)."""
    dev = _dev(qB, rB)
    counts = N.hamming_hist(_codes(qB, dev), _codes(rB, dev), rB.shape[1], _labels(query_L, dev), _labels(retrieval_L, dev))
    precision, recall = curves_from_counts(counts)
    return precision, recall, counts


def topn_precision(qB, rB, query_L, retrieval_L, topn=DEFAULT_TOPN):
    """-> (precision [len(topn)], recall [len(topn)], rel uint8 [Q, max(topn)] on the GPU) of the ranking's first N items."""
    dev = _dev(qB, rB)
    topn = [int(n) for n in topn]
    qp, rp = _codes(qB, dev), _codes(rB, dev)
    ql, rl = _labels(query_L, dev), _labels(retrieval_L, dev)
    _, _, rel, counts = N.hamming_topk(qp, rp, rB.shape[1], max(topn), ql, rl, want_counts=True)
    relevant = counts[:, :, 1].sum(1)
    precision, recall = topn_from_rel(rel, relevant, topn)
    return precision, recall, rel


class CodeIndex:
    """A database of hash codes, packed once.  search(query_codes, k) -> hamming_topk's tuple (graded=True: graded_topk's)."""

    def __init__(self, codes, labels=None):
        dev = _dev(codes)
        self.bits = codes.shape[1]
        self.size = codes.shape[0]
        self.planes = _codes(codes, dev)
        self.labels = _labels(labels, dev)
        self.classes = None if labels is None else labels.shape[1]
        self.device = dev

    @classmethod
    def from_mat(cls, path, side="r_img"):
        """The database side ("r_img" | "r_txt") of a file written by TrainBase.save_mat, with its labels r_l."""
        if side not in ("r_img", "r_txt"):
            raise ValueError(f"side {side!r}: r_img or r_txt")
        import scipy.io as scio
        m = scio.loadmat(path)
        labels = torch.from_numpy(m["r_l"]).float() if "r_l" in m else None
        return cls(torch.from_numpy(m[side]).float(), labels)

    def search(self, query_codes, k, query_labels=None, graded=False):
        if query_labels is not None and self.labels is None:
            raise N.NativeError("CodeIndex.search: query labels given, but the index has none")
        ql = _labels(query_labels, self.device)
        rl = self.labels if ql is not None else None
        if graded:
            if ql is None:
                raise N.NativeError("CodeIndex.search: graded=True needs query labels and an index with labels")
            return N.hamming_topk_graded(_codes(query_codes, self.device), self.planes, self.bits, k, ql, rl, classes=self.classes)
        idx, dist, rel = N.hamming_topk(_codes(query_codes, self.device), self.planes, self.bits, k, ql, rl)
        return (idx, dist) if rel is None else (idx, dist, rel)
