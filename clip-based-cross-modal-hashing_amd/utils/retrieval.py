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
The Q x N work runs in the kernels; reducing counts to curves is float64 arithmetic on small CPU tensors."""
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
    """A database of hash codes, packed once.  search(query_codes, k) -> hamming_topk's tuple."""

    def __init__(self, codes, labels=None):
        dev = _dev(codes)
        self.bits = codes.shape[1]
        self.size = codes.shape[0]
        self.planes = _codes(codes, dev)
        self.labels = _labels(labels, dev)
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

    def search(self, query_codes, k, query_labels=None):
        if query_labels is not None and self.labels is None:
            raise N.NativeError("CodeIndex.search: query labels given, but the index has none")
        ql = _labels(query_labels, self.device)
        rl = self.labels if ql is not None else None
        idx, dist, rel = N.hamming_topk(_codes(query_codes, self.device), self.planes, self.bits, k, ql, rl)
        return (idx, dist) if rel is None else (idx, dist, rel)
