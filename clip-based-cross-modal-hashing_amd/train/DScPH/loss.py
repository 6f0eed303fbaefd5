"""DScPH's proxy-fusion loss `CPF` (reference train/DScPH/CPF_loss.py:4-54) and the step's two quantisation terms (reference
train/DScPH/hash_train.py:64-70) as ONE native forward and one native backward launch (csrc/cpf.hip); nothing leaves the GPU.

    c = n(h) n(W)^T per modality;  tp = 2 sum max(c, 0) Y + b;  lp = sum (1 - c) exp((1 - c) sp) Y
    ln = sum_{c > tau} (c - psi) exp((c - mu) sn) (1 - Y);  L = 1 - tp / (tp + lp + ln);  CPF = L(image) + L(text)
    q = mean(sigma(z) (1 - sigma(z))), z = n(h);  step = CPF + quant_weight (q_img + q_txt)

What is decided here:
- the reference rotates the head outputs by a HouseHolder whose weights are the identity and sit in no optimiser group
  (hash_train.py:35-45): that rotation is X -> -X exactly and the q summand is even, so q is taken on n(h) itself; a trainable rotation
  is not built;
- the reference's label-smoothing branch is dead (ls_eps = 0, CPF_loss.py:15, :33) and is not built;
- the class proxies `weight` are a parameter of this module, trained by the step's own optimiser (its fourth BertAdam group) and, as
  in the reference, not part of the checkpoint."""
import torch

import cmh_native as N


class _CPF(torch.autograd.Function):
    """(loss [1], terms [4]) of (hi, ht, weight) under the labels; the terms are the log's and get no gradient"""

    @staticmethod
    def forward(ctx, hi, ht, weight, label, scalars, quant_weight):
        loss, terms, cos, saved = N.cpf_loss(hi, ht, label, weight, scalars, quant_weight, keep=True)
        ctx.saved = saved
        ctx.mark_non_differentiable(terms)
        return loss, terms

    @staticmethod
    def backward(ctx, dloss, _dterms):
        d_hi, d_ht, d_w = N.cpf_loss_backward(ctx.saved, dloss)
        return d_hi, d_ht, d_w, None, None, None


class CPFLoss(torch.nn.Module):
    def __init__(self, embed_dim, n_classes, tau=0.9, psi=0.7, sp=1.3, sn=1.3, mu=1.0, b=2.0, quant_weight=1.0):
        super(CPFLoss, self).__init__()
        self.in_features, self.out_features = int(embed_dim), int(n_classes)
        self.weight = torch.nn.Parameter(torch.empty(self.out_features, self.in_features))
        torch.nn.init.xavier_uniform_(self.weight)
        self.scalars = dict(tau=float(tau), psi=float(psi), sp=float(sp), sn=float(sn), mu=float(mu), b=float(b))
        self.quant_weight = float(quant_weight)

    def step_terms(self, image, text, labels):
        """-> the step's loss (0-dim: CPF + quant_weight (q_img + q_txt)) and its four terms [4] = L_img, L_txt, q_img, q_txt"""
        labels = labels.to(image.device).float()
        if torch.is_grad_enabled() and (image.requires_grad or text.requires_grad or self.weight.requires_grad):
            loss, terms = _CPF.apply(image, text, self.weight, labels, self.scalars, self.quant_weight)
        else:
            loss, terms = N.cpf_loss(image, text, labels, self.weight.detach(), self.scalars, self.quant_weight)[:2]
        return loss[0], terms

    def terms(self, image, text, labels):
        """the four terms alone, for the log and the tests"""
        return self.step_terms(image, text, labels)[1]

    def forward(self, image, text, labels):
        return self.step_terms(image, text, labels)[0]
