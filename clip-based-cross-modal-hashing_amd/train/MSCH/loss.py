"""Multi_Semantic_Correlation_Loss of DPSIH (reference train/DPSIH/Loss.py:78-137) as ONE native forward and one native backward
(csrc/msc.hip) for all the pairs of a step: the reference's [B, B, B] mask, its two gathers of up to B^3 / 4 indices and the length it
reads back on the host are one workgroup per anchor with two bit rows; nothing leaves the GPU.

What is decided here:
- with no active triplet the reference returns the integer 0 (:128-129); here that is a zero tensor with zero gradients;
- a triplet with s_an - s_ap == m exactly is counted (the mean's divisor) and adds nothing to a gradient: torch's relu'(0) is 0;
- the reference's trainer builds the loss with the STRING "all" and indexes it with 0 or 1 (:39, :115-116), so it reads the letter
  "a" or "l", never "semi-hard": it always mines `all`.  Both rules of :118-120 are built; `all` is the default;
- the reference clears the diagonal of `sames` whenever the mask is square (:107-108).  Both kinds of call of a step (:61) have B rows
  on either side, so the cross-modal call loses its diagonal too: an image's own caption is not one of its positives."""
import torch

import cmh_native as N


class _MSCLosses(torch.autograd.Function):
    """loss [n] of n (u, v) pairs over one label matrix: one forward call for all of them, one backward launch"""

    @staticmethod
    def forward(ctx, label, margin, mining, normalize, *codes):
        loss, count, sim, saved = N.msc_triplet_loss(list(zip(codes[0::2], codes[1::2])), label, margin, mining, normalize)
        ctx.saved = saved
        return loss

    @staticmethod
    def backward(ctx, dloss):
        grads = N.msc_triplet_loss_backward(ctx.saved, dloss)
        return (None, None, None, None) + tuple(g for pr in grads for g in pr)


def _wants_grad(tensors):
    return torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


class MSCLoss(torch.nn.Module):
    def __init__(self, margin=0.25, mining="all", normalize=False):
        super(MSCLoss, self).__init__()
        if mining not in N.MSC_MINING:
            raise ValueError(f"MSCLoss: mining {mining!r}: one of {sorted(N.MSC_MINING)}")
        self.margin, self.mining, self.normalize = float(margin), mining, bool(normalize)

    def losses(self, pairs, y):
        """f32 [n]: forward(u, v, y) of every (u, v) of `pairs` (at most four), in one call; `v is u` is the intra-modal call"""
        flat = [t for pr in pairs for t in pr]
        y = y.to(flat[0].device).float()
        if _wants_grad(flat):
            return _MSCLosses.apply(y, self.margin, self.mining, self.normalize, *flat)
        return N.msc_triplet_loss(pairs, y, self.margin, self.mining, self.normalize)[0]

    def forward(self, u, v, y):
        return self.losses([(u, v)], y)[0]
