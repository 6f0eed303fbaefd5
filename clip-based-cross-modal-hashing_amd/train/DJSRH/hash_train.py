"""DJSRH trainer (no upstream counterpart; paper: Su, Zhong, Zhang: Deep Joint-Semantics Reconstructing Hashing for Large-Scale
Unsupervised Cross-Modal Retrieval, ICCV 2019): label-free fine-tuning.  Model, optimiser groups and step are DSPH's; the loss is the
joint-semantics reconstruction of train/DJSRH/loss.py, whose target comes from the STOCK towers' features of the batch.  Those are
collected once, before the first step, into two f32 [N, D] tensors on the GPU (41 MB at 10 000 x 512) and gathered per step by the
`index` the loader yields, which is the item's row within the train split (dataset/base.py and dataset/synthetic.py return the
position __getitem__ was called with).  Labels are read by the evaluation alone.  The checkpoint has DSPH's keys.

Not built: several ranks (refused by name), refreshing the targets while the towers move, a frozen second copy of the towers."""
import os
import time

import torch

import dist_utils as du
from model.DJSRH import MDJSRH
from model.base.optimization import BertAdam
from train.base import TrainBase
from .get_args import INIT_HEADS, get_args
from .loss import JointSemanticsLoss


class DJSRHTrainer(TrainBase):

    def __init__(self, args, rank=0):
        args = get_args(args)
        args.rank = rank
        if du.world_size() > 1:      # before any data is touched
            raise NotImplementedError("DJSRH: the target cache is built on one rank (a sharded cache is not built); start it without "
                                      "torch.distributed.run")
        if args.init_heads not in INIT_HEADS:
            raise ValueError(f"DJSRH: --init-heads {args.init_heads}: one of {INIT_HEADS}")
        if not (0.0 <= args.djsrh_beta <= 1.0 and 0.0 <= args.djsrh_eta <= 1.0 and args.djsrh_mu > 0.0
                and args.djsrh_lambda1 >= 0.0 and args.djsrh_lambda2 >= 0.0):
            raise ValueError(f"DJSRH: --djsrh-beta {args.djsrh_beta} and --djsrh-eta {args.djsrh_eta} lie in [0, 1], --djsrh-mu "
                             f"{args.djsrh_mu} is positive, --djsrh-lambda1 {args.djsrh_lambda1} and --djsrh-lambda2 {args.djsrh_lambda2} "
                             "are not negative")
        super(DJSRHTrainer, self).__init__(args)
        self.logger.info("dataset len: {}".format(len(self.train_loader.dataset)))
        self.run()

    def _init_model(self):
        self.logger.info("init model.")
        self.model = MDJSRH(outputDim=self.args.output_dim, clipPath=self.args.clip_path,
                            writer=self.writer, logger=self.logger, is_train=self.args.is_train).to(self.rank)
        if self.args.pretrained != "" and os.path.exists(self.args.pretrained):
            self.logger.info("load pretrained model.")
            self.model.load_state_dict(torch.load(self.args.pretrained, map_location=f"cuda:{self.rank}"))
        self.model.float()
        self.model.clip.set_gemm_dtype(self.args.gemm_dtype)
        self.jsl = JointSemanticsLoss(self.args.djsrh_beta, self.args.djsrh_eta, self.args.djsrh_mu, self.args.djsrh_lambda1,
                                      self.args.djsrh_lambda2).to(self.rank)
        self.optimizer = BertAdam([
            {"params": self.model.clip.parameters(), "lr": self.args.clip_lr},
            {"params": self.model.image_hash.parameters(), "lr": self.args.lr},
            {"params": self.model.text_hash.parameters(), "lr": self.args.lr}],
            lr=self.args.lr, warmup=self.args.warmup_proportion, schedule="warmup_cosine", b1=0.9, b2=0.98, e=1e-6,
            t_total=len(self.train_loader) * self.args.epochs, weight_decay=self.args.weight_decay, max_grad_norm=1.0)
        self.cache_i = self.cache_t = None
        self.total_time = 0

    def collect_targets(self):
        """One pass without gradients over the train split: the towers' raw features, as loaded and before any step, f32 [N, D] on
        the GPU, row = the item's index.  The pass walks the train loader itself: with one rank _loader(data, train=False) builds the
        very same loader (the two differ under a DistributedSampler only), nothing is dropped, the order does not matter to a cache
        addressed by index, and a real dataset's device-resident image cache fills on the way instead of a second one being made.
        The image transform is the split's own (both chains are deterministic); where an item has several captions the cache holds
        the features of the one drawn in this pass."""
        began = time.time()
        n = len(self.train_loader.dataset)
        seen = torch.zeros(n, dtype=torch.bool, device=self.rank)
        with torch.no_grad():
            for batch in self.train_loader:
                image, text, index = batch[0].to(self.rank, non_blocking=True), batch[1].to(self.rank, non_blocking=True), batch[-1].to(self.rank)
                fi, ft = self.model.clip.encode_image(image).float(), self.model.clip.encode_text(text).float()
                if self.cache_i is None:
                    self.cache_i, self.cache_t = (torch.empty(n, fi.shape[1], dtype=torch.float32, device=self.rank) for _ in range(2))
                self.cache_i[index], self.cache_t[index] = fi, ft
                seen[index] = True
        if not bool(seen.all()):                                    # the pass's one read
            raise RuntimeError(f"DJSRH: the train loader left {int((~seen).sum())} of {n} items out of the target cache")
        self.total_time += time.time() - began
        self.logger.info(f">>>>>> target cache: {n} pairs, D = {self.cache_i.shape[1]}, "
                         f"{2 * self.cache_i.numel() * 4 / 1e6:.1f} MB, time: {self.total_time}")

    def init_heads(self):
        """--init-heads itq | cca: the training-free fit of utils/itq.py on the cached features, written into the heads"""
        if self.args.init_heads == "random":
            return
        from utils.itq import fit_hash_heads, load_heads
        fit = fit_hash_heads(self.cache_i, self.cache_t, self.args.output_dim, "cca" if self.args.init_heads == "cca" else "pca", "itq",
                             seed=self.args.seed)
        load_heads(self.model, fit)
        self.logger.info(f">>>>>> heads fitted: {self.args.init_heads} on {self.cache_i.shape[0]} pairs, scale = {float(fit['scale']):.6g}")

    def compute_loss(self, hash_img, hash_text, index):
        """-> loss and its three means, of the batch whose rows of the target cache `index` names"""
        S = self.jsl.target(self.cache_i[index], self.cache_t[index])
        return self.jsl.terms(hash_img, hash_text, S)

    def _step(self, image, text, index):
        """One optimisation step: DSPH's, with the label-free loss."""
        image, text, index = (t.to(self.rank, non_blocking=True) for t in (image, text, index))
        hash_img, hash_text = self.model(image, text)
        loss, terms = self.compute_loss(hash_img, hash_text, index)
        self.optimizer.zero_grad()
        self.backward(loss)
        self.optimizer.step()
        return loss.detach(), terms

    def train_epoch(self, epoch):
        self.change_state(mode="train")
        self.logger.info(">>>>>> epochs: %d/%d" % (epoch, self.args.epochs))
        all_loss, all_terms = 0, 0
        for image, text, label, index in self.train_loader:
            began = time.time()
            self.global_step += 1
            loss, terms = self._step(image, text, index)
            all_loss, all_terms = all_loss + loss, all_terms + terms
            self.total_time += time.time() - began
        steps = len(self.train_loader)
        ii, it, tt = (float(v) for v in (all_terms / steps).cpu())
        self.logger.info(f">>>>>> [{epoch}/{self.args.epochs}] loss: {all_loss.data / steps}, image-image: {ii:.6f}, image-text: {it:.6f}, "
                         f"text-text: {tt:.6f}, time: {self.total_time}")

    def train(self):
        self.change_state(mode="valid")
        self.collect_targets()
        self.init_heads()
        super(DJSRHTrainer, self).train()
