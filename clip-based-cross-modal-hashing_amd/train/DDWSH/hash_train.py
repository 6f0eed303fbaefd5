"""DDWSH trainer (reference train/DDWSH/hash_train.py): DSPH's model and step under the margin loss with distance-weighted triplets -
forward, sampler, loss, backward and optimiser on libcmh.  The per-class boundaries `beta` are the loss's parameter and BertAdam's
FOURTH group (reference :40-45); the checkpoint is the model's state alone (beta is not saved, as the reference's is not).

The registry calls the method DWSH (`--method DWSH`): `main.trainers["DDWSH"]` keeps raising NotImplementedError, which
tests/test_host.py pins, so the reference's method runs under this build's own name, as DScPH does under CPFH."""
import os
import time

import torch

from model.DDWSH import MDDWSH
from model.base.optimization import BertAdam
from train.base import TrainBase
from .get_args import SPACES, get_args
from .loss import MarginLoss


class DDWSHTrainer(TrainBase):

    def __init__(self, args, rank=0):
        args = get_args(args)
        args.rank = rank
        if args.dws_space not in SPACES:
            raise ValueError(f"DWSH: --dws-space {args.dws_space}: one of {SPACES}")
        super(DDWSHTrainer, self).__init__(args)
        self.logger.info("dataset len: {}".format(len(self.train_loader.dataset)))
        self.run()

    def _init_model(self):
        self.logger.info("init model.")
        self.model = MDDWSH(outputDim=self.args.output_dim, clipPath=self.args.clip_path,
                            writer=self.writer, logger=self.logger, is_train=self.args.is_train).to(self.rank)
        if self.args.pretrained != "" and os.path.exists(self.args.pretrained):
            self.logger.info("load pretrained model.")
            self.model.load_state_dict(torch.load(self.args.pretrained, map_location=f"cuda:{self.rank}"))
        self.model.float()
        self.model.clip.set_gemm_dtype(self.args.gemm_dtype)
        a = self.args
        self.criterion = MarginLoss(a.nclass, margin=a.dws_margin, beta=a.dws_beta, cutoff=a.dws_cutoff, space=a.dws_space,
                                    seed=a.dws_seed).to(self.rank)
        self.optimizer = BertAdam([
            {"params": self.model.clip.parameters(), "lr": self.args.clip_lr},
            {"params": self.model.image_hash.parameters(), "lr": self.args.lr},
            {"params": self.model.text_hash.parameters(), "lr": self.args.lr},
            {"params": self.criterion.parameters(), "lr": self.args.lr}],
            lr=self.args.lr, warmup=self.args.warmup_proportion, schedule="warmup_cosine", b1=0.9, b2=0.98, e=1e-6,
            t_total=len(self.train_loader) * self.args.epochs, weight_decay=self.args.weight_decay, max_grad_norm=1.0)
        self.total_time = 0

    def compute_loss(self, hash_img, hash_text, label, triplets=None):
        """L(img) + L(txt) + L(img, y=txt) (reference :68): one sampler call and one loss call for the three pairs"""
        return self.criterion(hash_img, hash_text, label, triplets)

    def _step(self, image, text, label):
        """One optimisation step."""
        image, text = image.to(self.rank, non_blocking=True), text.to(self.rank, non_blocking=True)
        label = label.to(self.rank, non_blocking=True).float()
        hash_img, hash_text = self.model(image, text)
        # several ranks: ONE fused all-gather of [B_local, 2K + C]: the triplets are drawn in the GLOBAL batch, by equal generators
        hash_img, hash_text, label = self.loss_inputs(hash_img, hash_text, label)
        loss = self.compute_loss(hash_img, hash_text, label)
        self.optimizer.zero_grad()
        self.backward(loss, self.criterion)       # + the gradient means over the ranks, beta's included
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
