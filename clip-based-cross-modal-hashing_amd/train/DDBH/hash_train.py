"""DDBH trainer (reference train/DDBH/hash_train.py:16-86; paper: Deep Discriminative Boundary Hashing for Cross-modal Retrieval,
TCSVT 2025): LinearHash heads on the CLIP towers, three base-point losses and two quantisation terms on the batch, fused BertAdam -
forward, loss, backward and optimiser on libcmh."""
import os
import time

import torch

from model.DDBH import MDDBH
from model.base.optimization import BertAdam
from train.base import TrainBase
from .get_args import get_args
from .loss import BPLoss, quantization_losses


class DDBHTrainer(TrainBase):

    def __init__(self, args, rank=0):
        args = get_args(args)
        args.rank = rank
        super(DDBHTrainer, self).__init__(args)
        self.logger.info("dataset len: {}".format(len(self.train_loader.dataset)))
        self.run()

    def _init_model(self):
        self.logger.info("init model.")
        self.model = MDDBH(outputDim=self.args.output_dim, clipPath=self.args.clip_path,
                           writer=self.writer, logger=self.logger, is_train=self.args.is_train).to(self.rank)
        if self.args.pretrained != "" and os.path.exists(self.args.pretrained):
            self.logger.info("load pretrained model.")
            self.model.load_state_dict(torch.load(self.args.pretrained, map_location=f"cuda:{self.rank}"))
        self.bp = BPLoss(bit=self.args.output_dim).to(self.rank)
        self.model.float()
        self.model.clip.set_gemm_dtype(self.args.gemm_dtype)
        self.optimizer = BertAdam([
            {"params": self.model.clip.parameters(), "lr": self.args.clip_lr},
            {"params": self.model.image_hash.parameters(), "lr": self.args.lr},
            {"params": self.model.text_hash.parameters(), "lr": self.args.lr}],
            lr=self.args.lr, warmup=self.args.warmup_proportion, schedule="warmup_cosine", b1=0.9, b2=0.98, e=1e-6,
            t_total=len(self.train_loader) * self.args.epochs, weight_decay=self.args.weight_decay, max_grad_norm=1.0)
        self.total_time = 0

    def compute_loss(self, hash_img, hash_text, label):
        """(intra image + intra text + inter) + 0.1 (image + text quantisation) (reference :64-78): the three base-point losses are
        one launch, the two quantisation terms another"""
        bp = self.bp.losses([(hash_img, hash_img), (hash_text, hash_text), (hash_img, hash_text)], label)
        q = quantization_losses([hash_img, hash_text], label)
        return (bp[0] + bp[1] + bp[2]) + 0.1 * (q[0] + q[1])

    def _step(self, image, text, label):
        """One optimisation step (reference :53-83)."""
        image, text = image.to(self.rank, non_blocking=True), text.to(self.rank, non_blocking=True)
        label = label.to(self.rank, non_blocking=True).float()
        hash_img, hash_text = self.model(image, text)
        # several ranks: ONE fused all-gather of [B_local, 2K + C]: inner, the indicator and each row's order statistics are B x B in
        # the GLOBAL batch
        hash_img, hash_text, label = self.loss_inputs(hash_img, hash_text, label)
        loss = self.compute_loss(hash_img, hash_text, label)
        self.optimizer.zero_grad()
        self.backward(loss)
        self.optimizer.step()
        return loss

    def train_epoch(self, epoch):
        self.change_state(mode="train")
        self.logger.info(">>>>>> epochs: %d/%d" % (epoch, self.args.epochs))
        all_loss = 0
        for image, text, label, index in self.train_loader:
            began = time.time()
            self.global_step += 1
            all_loss += self._step(image, text, label).detach()
            self.total_time += time.time() - began
        self.logger.info(f">>>>>> [{epoch}/{self.args.epochs}] loss: {all_loss.data / (len(self.train_loader))}, time: {self.total_time}")
