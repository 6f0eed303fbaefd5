"""BPLoss of DDBH (reference train/DDBH/loss.py:5-101) and the trainer's quantisation term (train/DDBH/hash_train.py:64-76), each as
ONE native forward and one native backward (csrc/ddbh.hip): the reference's Python walk over the batch, with two sorts and four
host reads per row, is one workgroup per row with a radix select; nothing leaves the GPU.

Departures from the reference, both decided: log(1 + e^-f) is evaluated as max(-f, 0) + log1p(e^-|f|), which does not overflow for
f < -88.7; a batch without any active row gives a zero tensor with zero gradients where the reference returns the integer 0.
(The reference's constructor names an unbound class in its super() call, :7; the class it means is its own.)"""
import torch

import cmh_native as N


class _BPLosses(torch.autograd.Function):
    """loss [n] of n (u, v) pairs over one label matrix: one forward launch for all of them, one backward launch"""

    @staticmethod
    def forward(ctx, label, scalars, *codes):
        loss, rows, count, pairs, label = N.ddbh_bp_loss(list(zip(codes[0::2], codes[1::2])), label, scalars)
        ctx.save_for_backward(label, rows, count, *[t for pr in pairs for t in pr])
        ctx.scalars = scalars
        return loss

    @staticmethod
    def backward(ctx, dloss):
        label, rows, count, *flat = ctx.saved_tensors
        grads = N.ddbh_bp_loss_backward(list(zip(flat[0::2], flat[1::2])), label, ctx.scalars, rows, count, dloss)
        return (None, None) + tuple(g for pr in grads for g in pr)


class _QuantLosses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, label, *hs):
        loss, colsum, hs = N.ddbh_quant_loss(list(hs), label)
        ctx.save_for_backward(colsum, *hs)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        colsum, *hs = ctx.saved_tensors
        return (None,) + tuple(N.ddbh_quant_loss_backward(hs, colsum, dloss))


def _wants_grad(tensors):
    return torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


class BPLoss(torch.nn.Module):
    def __init__(self, bit):
        super(BPLoss, self).__init__()
        self.y_p = 0.5
        self.right = bit / 6
        self.left = self.right / 2
        self.lowerBound = 0
        self.upperBound = bit / 4
        self.percent = 9 / 10

    def scalars(self):
        return (self.y_p, self.right, self.left, self.lowerBound, self.upperBound, self.percent)

    def losses(self, pairs, y):
        """f32 [n]: forward(u, v, y) of every (u, v) of `pairs` (at most four), in one launch"""
        flat = [t for pr in pairs for t in pr]
        y = y.to(flat[0].device).float()
        if _wants_grad(flat):
            return _BPLosses.apply(y, self.scalars(), *flat)
        return N.ddbh_bp_loss(pairs, y, self.scalars())[0]

    def forward(self, u, v, y):
        return self.losses([(u, v)], y)[0]


def quantization_losses(hs, label):
    """f32 [n]: mean(s @ (h - sign h)^2) of every h of `hs` (at most four), s = (label label^T > 0) as floats, in one launch"""
    hs = list(hs)
    label = label.to(hs[0].device).float()
    if _wants_grad(hs):
        return _QuantLosses.apply(label, *hs)
    return N.ddbh_quant_loss(hs, label)[0]


def quantization_loss(h, label):
    return quantization_losses([h], label)[0]
