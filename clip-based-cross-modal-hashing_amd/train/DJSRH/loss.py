"""The joint-semantics loss of DJSRH (Su, Zhong, Zhang: Deep Joint-Semantics Reconstructing Hashing, ICCV 2019; no upstream
counterpart), label-free: a target affinity S of the batch from the STOCK towers' image and caption features, and three
cosine-reconstruction terms that pull the codes' similarities (image-image, image-text, text-text) towards it - each as ONE native
forward and one native backward (csrc/djsrh.hip); nothing leaves the GPU.

    St = beta (2 cos(fi) - 1) + (1 - beta) (2 cos(ft) - 1),   S = mu ((1 - eta) St + (eta / B) St St^T)
    loss = lambda1 mean((b_I b_I^T - S)^2) + mean((b_I b_T^T - S)^2) + lambda2 mean((b_T b_T^T - S)^2),   b = F.normalize(h)

The five scalars' defaults are the paper's MIRFlickr settings as far as they are recalled: choices, not measured optima."""
import torch

import cmh_native as N


class _JointSemantics(torch.autograd.Function):
    """(loss [1], terms [3]) of (hi, ht) against S; S gets no gradient, and neither do the terms (they are the log's)"""

    @staticmethod
    def forward(ctx, hi, ht, S, lambda1, lambda2):
        loss, terms, tape, hi, ht = N.djsrh_loss(hi, ht, S, lambda1, lambda2, keep=True)
        ctx.save_for_backward(hi, ht, tape)
        ctx.lambdas = (lambda1, lambda2)
        ctx.mark_non_differentiable(terms)
        return loss, terms

    @staticmethod
    def backward(ctx, dloss, _dterms):
        hi, ht, tape = ctx.saved_tensors
        d_hi, d_ht = N.djsrh_loss_backward(hi, ht, tape, *ctx.lambdas, dloss)
        return d_hi, d_ht, None, None, None


class JointSemanticsLoss(torch.nn.Module):
    def __init__(self, beta=0.9, eta=0.4, mu=1.5, lambda1=0.1, lambda2=0.1):
        super(JointSemanticsLoss, self).__init__()
        self.beta, self.eta, self.mu, self.lambda1, self.lambda2 = float(beta), float(eta), float(mu), float(lambda1), float(lambda2)

    def scalars(self):
        return (self.beta, self.eta, self.mu, self.lambda1, self.lambda2)

    def target(self, fi, ft):
        """S f32 [B, B] from the stock features of the batch; never differentiated"""
        with torch.no_grad():
            return N.djsrh_target(fi.detach(), ft.detach(), self.beta, self.eta, self.mu)

    def terms(self, hi, ht, S):
        """-> loss (0-dim) and its three means [3] (image-image, image-text, text-text)"""
        S = S.detach()
        if torch.is_grad_enabled() and (hi.requires_grad or ht.requires_grad):
            loss, terms = _JointSemantics.apply(hi, ht, S, self.lambda1, self.lambda2)
        else:
            loss, terms = N.djsrh_loss(hi, ht, S, self.lambda1, self.lambda2)[:2]
        return loss[0], terms

    def forward(self, hi, ht, S):
        return self.terms(hi, ht, S)[0]
