"""DScPH trainer (reference train/DScPH/hash_train.py): DSPH's model and step under the proxy-fusion loss plus the two quantisation
terms - forward, loss, backward and optimiser on libcmh.  The class proxies are the loss's parameter and BertAdam's FOURTH group
(reference :37-44); the checkpoint is the model's state alone (the proxies are not saved, as the reference's are not).

The registry calls the method CPFH (`--method CPFH`): `main.trainers["DScPH"]` keeps raising NotImplementedError, which
tests/test_host.py pins, so the reference's method runs under this build's own name, as DPSIH's loss does under MSCH."""
import os
import time

import torch

from model.DScPH import MDScPH
from model.base.optimization import BertAdam
from train.base import TrainBase
from .get_args import get_args
from .loss import CPFLoss


class DScPHTrainer(TrainBase):

    def __init__(self, args, rank=0):
        args = get_args(args)
        args.rank = rank
        super(DScPHTrainer, self).__init__(args)
        self.logger.info("dataset len: {}".format(len(self.train_loader.dataset)))
        self.run()

    def _init_model(self):
        self.logger.info("init model.")
        self.model = MDScPH(outputDim=self.args.output_dim, clipPath=self.args.clip_path,
                            writer=self.writer, logger=self.logger, is_train=self.args.is_train).to(self.rank)
        if self.args.pretrained != "" and os.path.exists(self.args.pretrained):
            self.logger.info("load pretrained model.")
            self.model.load_state_dict(torch.load(self.args.pretrained, map_location=f"cuda:{self.rank}"))
        self.model.float()
        self.model.clip.set_gemm_dtype(self.args.gemm_dtype)
        a = self.args
        self.cpf = CPFLoss(a.output_dim, a.nclass, tau=a.cpf_tau, psi=a.cpf_psi, sp=a.cpf_sp, sn=a.cpf_sn, mu=a.cpf_mu, b=a.cpf_b,
                           quant_weight=a.quant_weight).to(self.rank)
        self.optimizer = BertAdam([
            {"params": self.model.clip.parameters(), "lr": self.args.clip_lr},
            {"params": self.model.image_hash.parameters(), "lr": self.args.lr},
            {"params": self.model.text_hash.parameters(), "lr": self.args.lr},
            {"params": self.cpf.parameters(), "lr": self.args.lr}],
            lr=self.args.lr, warmup=self.args.warmup_proportion, schedule="warmup_cosine", b1=0.9, b2=0.98, e=1e-6,
            t_total=len(self.train_loader) * self.args.epochs, weight_decay=self.args.weight_decay, max_grad_norm=1.0)
        self.total_time = 0

    def compute_loss(self, hash_img, hash_text, label):
        """-> (CPF + quant_weight (q_img + q_txt), the CPF part alone for the log): one native call (reference :64-70)"""
        loss, terms = self.cpf.step_terms(hash_img, hash_text, label)
        return loss, terms[0] + terms[1]

    def _step(self, image, text, label):
        """One optimisation step; returns the CPF part, which is what the reference's epoch log adds up (:72)."""
        image, text = image.to(self.rank, non_blocking=True), text.to(self.rank, non_blocking=True)
        label = label.to(self.rank, non_blocking=True).float()
        hash_img, hash_text = self.model(image, text)
        # several ranks: ONE fused all-gather of [B_local, 2K + C]: the loss's sums are taken over the GLOBAL batch
        hash_img, hash_text, label = self.loss_inputs(hash_img, hash_text, label)
        loss, cpf_part = self.compute_loss(hash_img, hash_text, label)
        self.optimizer.zero_grad()
        self.backward(loss, self.cpf)             # + the gradient means over the ranks, the proxies' included
        self.optimizer.step()
        return cpf_part

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
