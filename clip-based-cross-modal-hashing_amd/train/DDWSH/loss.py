"""DDWSH's `MarginLoss` with its `DistanceWeightedMiner` (reference train/DDWSH/loss.py:7-128) for the three calls of a step
(train/DDWSH/hash_train.py:68) as ONE native forward and one native backward (csrc/dws.hip): the reference's label copy to the host,
its Python loop over the anchors, the row it reads back per anchor and its two numpy draws per anchor are one workgroup per anchor;
nothing leaves the GPU.

What is decided here:
- the reference's `forward` reads `self.beta_constant`, which nothing sets: it runs only with that attribute set to False from outside,
  which is the branch built (per-class boundaries, averaged over an anchor's labels, :34-37);
- the reference hands the miner the distance matrix as its batch (:22), so it mines on the distances between the ROWS of D with
  dim = B: `space="distances"`, the default.  `space="embeddings"` mines on D itself with dim = K, which is what Wu et al. describe;
- the contrastive branch never fires (contrastive_p = 0, :87) and upper_cutoff, tau and gamma are never read: none is built;
- the sampler's uniforms are drawn by torch from ONE generator per module, seeded from `seed`: a run is repeatable and every rank of a
  multi-GPU run draws the same numbers for the same (gathered) batch.  The draws are not numpy's, so triplets differ from the
  reference's for equal seeds; the tests hand the reference's triplets in;
- a pair without a valid anchor gives a loss of 0 with zero gradients; the reference returns the tuple (0, 0) there (:24-26), which its
  step cannot add to a tensor loss."""
import torch

import cmh_native as N


class _DWSLosses(torch.autograd.Function):
    """loss [n] of n (u, v) pairs over one label matrix and one beta, on given triplets: one forward, one backward"""

    @staticmethod
    def forward(ctx, label, beta, triplets, margin, pre, *codes):
        loss, count, dist, saved = N.dws_margin_loss(list(zip(codes[0::2], codes[1::2])), label, beta, triplets, margin, pre)
        ctx.saved = saved
        return loss

    @staticmethod
    def backward(ctx, dloss):
        grads, dbeta = N.dws_margin_loss_backward(ctx.saved, dloss)
        return (None, dbeta, None, None, None) + tuple(g for pr in grads for g in pr)


class MarginLoss(torch.nn.Module):
    def __init__(self, nclass, margin=0.2, beta=1.2, cutoff=0.5, space="distances", seed=0):
        super(MarginLoss, self).__init__()
        if space not in N.DWS_SPACES:
            raise ValueError(f"MarginLoss: space {space!r}: one of {sorted(N.DWS_SPACES)}")
        self.margin, self.cutoff, self.space, self.seed = float(margin), float(cutoff), space, int(seed)
        self.beta = torch.nn.Parameter(torch.ones(int(nclass)) * float(beta))
        self.generator = None                                     # made on the first draw, on the device of the codes

    def uniforms(self, n, B, device):
        """f32 [n, B, 2] in [0, 1): (u_p, u_n) per anchor and pair, the next draws of this module's generator"""
        if self.generator is None or self.generator.device != torch.device(device):
            self.generator = torch.Generator(device=device)
            self.generator.manual_seed(self.seed)
        return torch.rand(n, B, 2, generator=self.generator, device=device, dtype=torch.float32)

    def _mine(self, pairs, label, uniforms, weights):
        """-> triplets, weights or None, and the distances they were drawn on (what N.dws_distances returns); no gradient"""
        with torch.no_grad():
            pre = N.dws_distances(pairs)
            B, K = pre[1][0][0][0].shape
            if uniforms is None:
                uniforms = self.uniforms(len(pairs), B, pre[0].device)
            trip, w = N.dws_mine(pre[0], label.to(pre[0].device).float(), K, uniforms, self.cutoff, self.space, weights)
        return trip, w, pre

    def mine(self, pairs, label, uniforms=None, weights=False):
        """-> triplets i32 [n, B, 2] (and the weights f64 [n, B, B] with `weights`) of the pairs"""
        trip, w, _ = self._mine(pairs, label, uniforms, weights)
        return (trip, w) if weights else trip

    def losses(self, pairs, label, triplets=None):
        """f32 [n]: forward(u, label, v) of every (u, v) of `pairs` (at most three); `v is u` is the intra-modal call"""
        flat = [t for pr in pairs for t in pr]
        label = label.to(flat[0].device).float()
        pre = None
        if triplets is None:                                      # (the loss then takes the distances the sampler ran on: one walk)
            triplets, _, pre = self._mine(pairs, label, None, False)
        if torch.is_grad_enabled() and (self.beta.requires_grad or any(t.requires_grad for t in flat)):
            return _DWSLosses.apply(label, self.beta, triplets, self.margin, pre, *flat)
        return N.dws_margin_loss(pairs, label, self.beta.detach(), triplets, self.margin, pre)[0]

    def forward(self, hash_img, hash_text, label, triplets=None):
        """L(img) + L(txt) + L(img, y=txt) (reference train/DDWSH/hash_train.py:68); triplets i32 [3, B, 2] may be handed in"""
        return self.losses([(hash_img, hash_img), (hash_text, hash_text), (hash_img, hash_text)], label, triplets).sum()
