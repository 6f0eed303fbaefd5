"""Code diagnostics: what is wrong with a set of hash codes when the mAP comes out low.

    bits balanced?                 bit_bias, balance, bit_entropy
    bits independent?              corr, mean_abs_corr, max_abs_corr, dead_bits, duplicate_bits
    image and caption code agree?  (paired=) pair_dot, bit_agreement, mean_agreement, pair_distance, cross_corr
    which bit carries which class? (labels=) class_bit_mean, bit_class_mi, best_class

Every answer is made of sums over the database of products of two bit columns.  code_gram gets those integers from the packed planes
on the GPU (cmh_code_gram: exact int64, no float copy of the codes, any N up to 2^31 - 1); stats_from_counts turns them into the
statistics on the host, in float64 and - where a decision is exact (dead, duplicate) - in Python integers.  The integers are in the
result ("gram", "sum", "abs", ...): a caller who shards the database over ranks adds them and calls stats_from_counts once."""
import math
from collections import namedtuple

import numpy as np

Operand = namedtuple("Operand", "planes bits")      # (sign, nz) int32 [N, ceil(bits / 32)] on the GPU, and the bits that count


def operand(x, kind="codes"):
    """-> Operand.  x: f32 codes [N, K] in {-1, 0, +1}, a (sign, nz) pair of planes (bits = 32 per word unless x is an Operand), a
    CodeIndex, or an Operand.  kind="labels": x is multi-hot [N, C], packed by pack_labels (entries 0 / 1).  kind="abs": |code|, the
    operand's nz plane as both planes."""
    import torch

    import cmh_native as N
    if kind == "labels":
        if isinstance(x, torch.Tensor) and x.dtype != torch.int32:
            from utils.retrieval import _dev
            lab = N.pack_labels(x.to(_dev(x)).float())
            return Operand((lab, lab), x.shape[1])
        raise N.NativeError("code_stats.operand: labels are a multi-hot tensor [N, C]")
    if isinstance(x, Operand):
        op = x
    elif isinstance(x, torch.Tensor):
        from utils.retrieval import _dev
        if x.dim() != 2:
            raise N.NativeError(f"code_stats.operand: codes [N, K], not {tuple(x.shape)}")
        op = Operand(N.pack_codes(x.to(_dev(x)).float()), x.shape[1])
    elif isinstance(x, tuple) and len(x) == 2:
        op = Operand((x[0].contiguous(), x[1].contiguous()), 32 * x[0].shape[1])
    elif hasattr(x, "planes") and hasattr(x, "bits"):      # a CodeIndex
        op = Operand(tuple(t.contiguous() for t in x.planes), x.bits)
    else:
        raise N.NativeError(f"code_stats.operand: codes, a (sign, nz) pair, a CodeIndex or an Operand, not {type(x).__name__}")
    return Operand((op.planes[1], op.planes[1]), op.bits) if kind == "abs" else op


def code_gram(A, B=None, chunk_items=0):
    """-> (gram int64 [abits, bbits], a_sum, a_abs int64 [abits], b_sum, b_abs int64 [bbits]) on the GPU: gram[i][j] = sum over the
    items of a_i b_j, the sums of a_i, |a_i|, b_j, |b_j|.  A, B: whatever operand() takes; B=None: B is A."""
    import cmh_native as N
    a = operand(A)
    b = a if B is None else operand(B)
    if a.planes[0].shape[0] != b.planes[0].shape[0]:
        raise N.NativeError(f"code_gram: the operands hold {a.planes[0].shape[0]} and {b.planes[0].shape[0]} items")
    return N.code_gram(a.planes, b.planes, a.bits, b.bits, chunk_items)


def _ints(x):
    """Anything that holds integers (tensor, array, nested list) -> nested lists of Python ints."""
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=object).tolist() if not isinstance(x, np.ndarray) else x.astype(object).tolist()


def _f(x):
    return np.array(x, dtype=object).astype(np.float64)


def _plogp(p):
    """p log2 p with 0 log 0 = 0."""
    p = np.asarray(p, dtype=np.float64)
    out = np.zeros_like(p)
    nz = p > 0
    out[nz] = p[nz] * np.log2(p[nz])
    return out


def _corr(n, gram, s_a, v_a, s_b, v_b):
    """Pearson's correlation from the integers: D_ij / sqrt(V_i V_j), D_ij = n gram_ij - s_i s_j, V_i = n ab_i - s_i^2 (a_i^2 = |a_i|);
    0 where either variance is 0.  D and V are exact Python integers (up to 2^124), rounded to float64 once."""
    D = _f([[n * gram[i][j] - s_a[i] * s_b[j] for j in range(len(s_b))] for i in range(len(s_a))]).reshape(len(s_a), len(s_b))
    ra, rb = np.sqrt(_f(v_a)), np.sqrt(_f(v_b))
    den = ra[:, None] * rb[None, :]
    return np.divide(D, den, out=np.zeros_like(D), where=den > 0), D


def stats_from_counts(n, gram, s, ab, *, pair=None, classes=None):
    """The statistics of K-bit codes over n items from their integers: gram [K, K] = sum a_i a_j, s [K] = sum a_i, ab [K] = sum |a_i|.
    pair = (gram_xy [K, K2], s2 [K2], ab2 [K2]): this side against the other modality's codes of the same items, and that side's
    sums.  classes = (count [C], gram_lc [C, K], gram_la [C, K]): the class sizes, gram(label, code) and gram(label, |code|).
    Pure host arithmetic -> a dict (arrays are numpy)."""
    n = int(n)
    gram, s, ab = _ints(gram), _ints(s), _ints(ab)
    K = len(s)
    if n < 1 or len(gram) != K or any(len(r) != K for r in gram) or len(ab) != K:
        raise ValueError(f"stats_from_counts: n={n}, gram {len(gram)} rows, s {K}, ab {len(ab)}")
    V = [n * gram[i][i] - s[i] * s[i] for i in range(K)]           # n^2 times the variance: exact
    dead = [i for i in range(K) if V[i] == 0]
    live = [i for i in range(K) if V[i] != 0]
    sf, af = _f(s), _f(ab)
    mean = sf / n
    ent = -(_plogp((af + sf) / (2.0 * n)) + _plogp((af - sf) / (2.0 * n)) + _plogp(1.0 - af / n))
    corr, _ = _corr(n, gram, s, V, s, V)
    for i in live:
        corr[i, i] = 1.0
    best, best_pair, total, pairs, dup = 0.0, None, 0.0, 0, []
    for x, i in enumerate(live):
        for j in live[x + 1:]:
            c = abs(corr[i, j])
            total, pairs = total + c, pairs + 1
            if best_pair is None or c > best:
                best, best_pair = c, (i, j)
            d = n * gram[i][j] - s[i] * s[j]
            if d * d == V[i] * V[j]:                                # |corr| == 1 exactly: a copy or a negation
                dup.append((i, j))
    out = {"n": n, "bits": K, "gram": np.array(gram, dtype=np.int64).reshape(K, K), "sum": np.array(s, dtype=np.int64),
           "abs": np.array(ab, dtype=np.int64), "bit_mean": mean, "bit_bias": np.abs(mean), "balance": float(np.abs(mean).mean()),
           "bit_entropy": ent, "dead_bits": dead, "corr": corr, "mean_abs_corr": total / pairs if pairs else 0.0,
           "max_abs_corr": float(best), "max_corr_pair": best_pair, "duplicate_bits": dup}
    if pair is not None:
        gxy, s2, ab2 = _ints(pair[0]), _ints(pair[1]), _ints(pair[2])
        K2 = len(s2)
        if len(gxy) != K or any(len(r) != K2 for r in gxy) or len(ab2) != K2:
            raise ValueError("stats_from_counts: pair = (gram_xy [K, K2], s2 [K2], ab2 [K2])")
        V2 = [n * ab2[j] - s2[j] * s2[j] for j in range(K2)]
        dot = [gxy[k][k] for k in range(min(K, K2))]
        df = _f(dot)
        out.update({"pair_gram": np.array(gxy, dtype=np.int64).reshape(K, K2), "pair_sum": np.array(s2, dtype=np.int64),
                    "pair_abs": np.array(ab2, dtype=np.int64), "pair_dot": np.array(dot, dtype=np.int64),
                    "bit_agreement": (1.0 + df / n) / 2.0, "mean_agreement": float(((1.0 + df / n) / 2.0).mean()),
                    "pair_distance": 0.5 * (len(dot) - float(math.fsum((df / n).tolist()))),
                    "cross_corr": _corr(n, gxy, s, V, s2, V2)[0]})
    if classes is not None:
        cnt, glc, gla = _ints(classes[0]), _ints(classes[1]), _ints(classes[2])
        C = len(cnt)
        if len(glc) != C or len(gla) != C or any(len(r) != K for r in glc) or any(len(r) != K for r in gla):
            raise ValueError("stats_from_counts: classes = (count [C], gram_lc [C, K], gram_la [C, K])")
        cf, lc, la = _f(cnt)[:, None], _f(glc).reshape(C, K), _f(gla).reshape(C, K)
        cbm = np.divide(lc, cf, out=np.zeros_like(lc), where=cf > 0)
        # the 3 x 2 table of symbol (+, -, 0) against membership (1, 0), per class and bit
        sym = np.stack([(af + sf) / 2.0, (af - sf) / 2.0, n - af])                  # [3, K]: n(+), n(-), n(0)
        inside = np.stack([(la + lc) / 2.0, (la - lc) / 2.0, cf - la])              # [3, C, K]: n(s, 1)
        mi = np.zeros((C, K))
        for table, members in ((inside, cf), (sym[:, None, :] - inside, n - cf)):
            marg = sym[:, None, :] * members[None, :, :]                            # n(s) n(m)
            ok = (table > 0) & (marg > 0)
            ratio = np.divide(table * n, marg, out=np.ones_like(table), where=ok)
            mi += np.where(ok, table / n * np.log2(ratio), 0.0).sum(0)
        out.update({"class_count": np.array(cnt, dtype=np.int64), "class_gram": np.array(glc, dtype=np.int64).reshape(C, K),
                    "class_abs_gram": np.array(gla, dtype=np.int64).reshape(C, K), "class_bit_mean": cbm, "bit_class_mi": mi,
                    "best_class": mi.argmax(0), "best_class_mi": mi.max(0)})
    return out


def code_stats(codes, labels=None, paired=None, chunk_items=0):
    """The diagnostics of one set of codes (whatever operand() takes; a CodeIndex brings its labels when labels is None) -> the dict
    of stats_from_counts.  paired: the other modality's codes of the same items; labels: multi-hot [N, C].  Two to four
    cmh_code_gram calls; the integers come to the host once."""
    a = operand(codes)
    n = a.planes[0].shape[0]
    if paired is None:
        gram, s, ab, _, _ = code_gram(a, chunk_items=chunk_items)
        pair = None
    else:
        gram, s, ab = code_gram(a, chunk_items=chunk_items)[:3]
        gxy, _, _, s2, ab2 = code_gram(a, paired, chunk_items=chunk_items)
        pair = (gxy.cpu(), s2.cpu(), ab2.cpu())
    lab = None
    if labels is not None:
        lab = operand(labels, "labels")
    elif getattr(codes, "labels", None) is not None and getattr(codes, "classes", None):      # a CodeIndex with labels
        lab = Operand((codes.labels.contiguous(), codes.labels.contiguous()), codes.classes)
    classes = None
    if lab is not None:
        glc, cnt = code_gram(lab, a, chunk_items=chunk_items)[:2]
        gla = code_gram(lab, operand(a, "abs"), chunk_items=chunk_items)[0]
        classes = (cnt.cpu(), glc.cpu(), gla.cpu())
    return stats_from_counts(n, gram.cpu(), s.cpu(), ab.cpu(), pair=pair, classes=classes)


def bucket_stats_from_sizes(n, sizes, size_counts, bits=None):
    """How n items spread over their distinct codes, from the occupancy table of a BucketTable: sizes = the distinct bucket sizes,
    size_counts = how many buckets have each (torch.unique(counts, return_counts=True): at most about sqrt(2 n) rows).  Pure host
    arithmetic; the counts are exact Python integers -> a dict:
      distinct, singletons, largest; collisions = sum n_b (n_b - 1) / 2, the pairs of items with equal codes;
      collision_probability = sum n_b^2 / n^2, the chance that two items drawn with replacement share a code;
      bucket_entropy_bits = -sum (n_b / n) log2 (n_b / n) (float64); occupancy = int64 [rows, 2] (size, buckets), ascending by size;
      with bits (the code length): bits and used_share = distinct / min(n, 2^bits), the share of the codes the items could occupy
      that they do."""
    n = int(n)
    table = sorted(zip((int(s) for s in _ints(sizes)), (int(c) for c in _ints(size_counts))))
    if n < 1 or not table or any(s < 1 or c < 1 for s, c in table) or sum(s * c for s, c in table) != n \
            or len({s for s, _ in table}) != len(table):
        raise ValueError(f"bucket_stats_from_sizes: (size, buckets) rows of distinct sizes >= 1 that add up to n={n}")
    shares = np.array([s for s, _ in table], dtype=np.float64) / n
    out = {"n": n, "distinct": sum(c for _, c in table), "singletons": sum(c for s, c in table if s == 1), "largest": table[-1][0],
           "collisions": sum(c * (s * (s - 1) // 2) for s, c in table),
           "collision_probability": sum(c * s * s for s, c in table) / (n * n),
           "bucket_entropy_bits": float(-(np.array([c for _, c in table], dtype=np.float64) * _plogp(shares)).sum()),
           "occupancy": np.array(table, dtype=np.int64).reshape(-1, 2)}
    if bits is not None:
        out["bits"] = int(bits)
        out["used_share"] = out["distinct"] / min(n, 1 << int(bits))
    return out


def bucket_summary_lines(name, st):
    """The bucket statistics as lines of text (retrieve.py --bucket-stats)."""
    top = st["occupancy"][-3:][::-1]
    return [f"{name}: {st['n']} items x {st['bits']} bit  distinct {st['distinct']}  singletons {st['singletons']}  largest {st['largest']}  "
            f"used share {st['used_share']:.6f}",
            f"{name}: collisions {st['collisions']}  collision probability {st['collision_probability']:.6e}  "
            f"bucket entropy {st['bucket_entropy_bits']:.6f} bit  largest sizes " + " ".join(f"{int(s)}x{int(c)}" for s, c in top)]


def summary_lines(name, st, top=3):
    """The short table of retrieve.py --stats and the trainer's log, as lines of text."""
    pair = st["max_corr_pair"]
    lines = [f"{name}: {st['n']} items x {st['bits']} bit  balance {st['balance']:.6f}  entropy {float(st['bit_entropy'].mean()):.6f}  "
             f"dead {st['dead_bits']}  duplicates {st['duplicate_bits']}",
             f"{name}: mean|corr| {st['mean_abs_corr']:.6f}  max|corr| {st['max_abs_corr']:.6f}" + (f" at bits {pair[0]},{pair[1]}" if pair else "")]
    if "bit_agreement" in st:
        worst = np.argsort(st["bit_agreement"], kind="stable")[:top]
        lines.append(f"{name}: pair agreement {st['mean_agreement']:.6f}  distance {st['pair_distance']:.6f}  least agreeing bits "
                     + " ".join(f"{int(k)}:{st['bit_agreement'][k]:.4f}" for k in worst))
    if "bit_class_mi" in st:
        lines.append(f"{name}: bit:class:MI " + " ".join(f"{k}:{int(c)}:{m:.4f}" for k, (c, m) in enumerate(zip(st["best_class"], st["best_class_mi"]))))
    return lines


def arrays(st, prefix=""):
    """The arrays and numbers of a stats dict under prefixed names, for np.savez / save_mat (lists become arrays, None is left out)."""
    out = {}
    for key, v in st.items():
        if v is None:
            continue
        if key in ("dead_bits", "max_corr_pair"):
            v = np.array(v, dtype=np.int64)
        elif key == "duplicate_bits":
            v = np.array(v, dtype=np.int64).reshape(-1, 2)
        out[prefix + key] = np.asarray(v)
    return out
