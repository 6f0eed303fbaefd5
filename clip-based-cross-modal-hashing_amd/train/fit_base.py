"""What the training-free trainers (train/ITQ, train/DCH) share: one rank, a model whose heads the fit writes, one pass over the train
loader without gradients that keeps the towers' features (and their running moments) on the GPU, and train() = fit, validate, save
model-0.pth.  A method subclasses FitTrainer, names itself and its model class, checks its own arguments and writes fit()."""
import os

import torch

import dist_utils as du
from train.base import TrainBase
from utils.itq import MomentStream


class FitTrainer(TrainBase):
    name = None             # the method, as it stands in refusals
    model_class = None      # Baseclip with LinearHash heads

    def __init__(self, args, rank=0):
        """args: the method's own get_args(args)"""
        args.rank = rank
        self.check_args(args)
        if du.world_size() > 1:      # before any data is touched
            raise NotImplementedError(f"{self.name}: the fit runs on one rank (a sharded fit is not built); start it without torch.distributed.run")
        super().__init__(args)
        self.logger.info("dataset len: {}".format(len(self.train_loader.dataset)))
        self.run()

    @staticmethod
    def check_args(args):
        """ValueError for a flag the fit would refuse, before any data is touched"""

    def _init_model(self):
        self.logger.info("init model.")
        self.model = self.model_class(outputDim=self.args.output_dim, clipPath=self.args.clip_path,
                                      writer=self.writer, logger=self.logger, is_train=self.args.is_train).to(self.rank)
        if self.args.pretrained != "" and os.path.exists(self.args.pretrained):
            self.logger.info("load pretrained model.")
            self.model.load_state_dict(torch.load(self.args.pretrained, map_location=f"cuda:{self.rank}"))
        self.model.float()
        self.model.clip.set_gemm_dtype(self.args.gemm_dtype)
        self.total_time = 0

    def collect_features(self, keep_labels=False, cross=False):
        """One pass over the train loader: the towers' raw features of up to --fit-num items (all of them by default), f32 on the
        GPU, with keep_labels their labels too (else None), and the features' running moments (with `cross` the cross moments
        too), one batch per call -> Fi, Ft, Y, moments."""
        limit = int(self.args.fit_num) if int(self.args.fit_num) > 0 else None
        feats_i, feats_t, labels, moments, seen = [], [], [], MomentStream(cross=cross), 0
        with torch.no_grad():
            for batch in self.train_loader:
                items = [t.to(self.rank, non_blocking=True) for t in batch[:3 if keep_labels else 2]]
                if limit is not None and seen + items[0].shape[0] > limit:
                    items = [t[:limit - seen] for t in items]
                fi, ft = self.model.clip.encode_image(items[0]).float(), self.model.clip.encode_text(items[1]).float()
                moments.add(fi, ft)
                feats_i.append(fi)
                feats_t.append(ft)
                if keep_labels:
                    labels.append(items[2].float())
                seen += fi.shape[0]
                if limit is not None and seen >= limit:
                    break
        return torch.cat(feats_i), torch.cat(feats_t), torch.cat(labels) if keep_labels else None, moments

    def fit(self):
        """Collect, fit, load the heads into self.model, log, keep the record in self.last_fit and return it."""
        raise NotImplementedError

    def train(self):
        self.logger.info("Start fit.")
        self.fit()
        self.valid(0)
        self.save_model(0)
        self.logger.info(
            f">>>>>>> FINISHED >>>>>> Best epoch, I-T: {self.best_epoch_i}, mAP: {self.max_mapi2t}, T-I: {self.best_epoch_t}, mAP: {self.max_mapt2i}")
