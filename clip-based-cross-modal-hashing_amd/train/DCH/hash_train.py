"""Supervised training-free codes from a stock CLIP checkpoint (no upstream counterpart): discrete cross-modal hashing (DCH, Xu et
al., TIP 2017) on the towers' own features.  train() makes one pass over the train loader without gradients, keeps the features and
the labels of the fit set on the GPU, fits the two heads (utils/dch.py, csrc/dch.hip), writes them into the model, saves model-0.pth
and runs the usual validation.  The checkpoint has DSPH's keys: it loads as `--method DCH`, as `--method ITQ` and as `--method DSPH`."""
import os
import time

import torch

import dist_utils as du
from model.DCH import MDCH
from train.base import TrainBase
from utils.dch import fit_from_moments, supervised_moments
from utils.itq import MomentStream, load_heads
from .get_args import get_args


class DCHTrainer(TrainBase):

    def __init__(self, args, rank=0):
        args = get_args(args)
        args.rank = rank
        if args.dch_iters < 0 or args.dch_rounds < 1:
            raise ValueError(f"DCH: --dch-iters {args.dch_iters} / --dch-rounds {args.dch_rounds}: need iters >= 0 and rounds >= 1")
        if not (args.dch_lambda > 0.0 and args.dch_mu >= 0.0 and args.dch_reg > 0.0):
            raise ValueError(f"DCH: --dch-lambda {args.dch_lambda} / --dch-mu {args.dch_mu} / --dch-reg {args.dch_reg}: "
                             f"need lambda > 0, mu >= 0 and reg > 0")
        if du.world_size() > 1:      # before any data is touched
            raise NotImplementedError("DCH: the fit runs on one rank (a sharded fit is not built); start it without torch.distributed.run")
        super(DCHTrainer, self).__init__(args)
        self.logger.info("dataset len: {}".format(len(self.train_loader.dataset)))
        self.run()

    def _init_model(self):
        self.logger.info("init model.")
        self.model = MDCH(outputDim=self.args.output_dim, clipPath=self.args.clip_path,
                          writer=self.writer, logger=self.logger, is_train=self.args.is_train).to(self.rank)
        if self.args.pretrained != "" and os.path.exists(self.args.pretrained):
            self.logger.info("load pretrained model.")
            self.model.load_state_dict(torch.load(self.args.pretrained, map_location=f"cuda:{self.rank}"))
        self.model.float()
        self.model.clip.set_gemm_dtype(self.args.gemm_dtype)
        self.total_time = 0

    def collect_features(self):
        """One pass over the train loader: the towers' raw features and the labels of up to --fit-num items (all of them by
        default), f32 on the GPU, and the features' running moments, one batch per call."""
        limit = int(self.args.fit_num) if int(self.args.fit_num) > 0 else None
        feats_i, feats_t, labels, moments, seen = [], [], [], MomentStream(), 0
        with torch.no_grad():
            for batch in self.train_loader:
                image, text = batch[0].to(self.rank, non_blocking=True), batch[1].to(self.rank, non_blocking=True)
                label = batch[2].to(self.rank, non_blocking=True)
                if limit is not None and seen + image.shape[0] > limit:
                    image, text, label = image[:limit - seen], text[:limit - seen], label[:limit - seen]
                fi, ft = self.model.clip.encode_image(image).float(), self.model.clip.encode_text(text).float()
                moments.add(fi, ft)
                feats_i.append(fi)
                feats_t.append(ft)
                labels.append(label.float())
                seen += fi.shape[0]
                if limit is not None and seen >= limit:
                    break
        return torch.cat(feats_i), torch.cat(feats_t), torch.cat(labels), moments

    def fit(self):
        began = time.time()
        self.change_state(mode="valid")
        Fi, Ft, Y, moments = self.collect_features()
        a = self.args
        fit = fit_from_moments(Fi, Ft, Y, supervised_moments(moments), a.output_dim, a.dch_iters, a.dch_rounds, a.dch_lambda, a.dch_mu,
                               a.dch_reg)
        load_heads(self.model, fit)
        self.total_time += time.time() - began
        obj = [float(v) for v in fit["objective"].cpu()]                 # the fit's reads: after the last launch
        flips, margins, info = fit["flips"].cpu().tolist(), fit["min_margin"].cpu().tolist(), fit["solve_info"].cpu().tolist()
        self.logger.info(f">>>>>> fit: DCH on {Fi.shape[0]} pairs, D = {Fi.shape[1]}, C = {Y.shape[1]}, bits = {a.output_dim}, "
                         f"lambda = {a.dch_lambda:g}, mu = {a.dch_mu:g}, reg = {a.dch_reg:g} / D, scale = {float(fit['scale']):.6g}, "
                         f"time: {self.total_time}")
        self.logger.info(f">>>>>> Jacobi sweeps (S_ii, S_tt, C): {fit['eigh_sweeps']}, converged: {fit['eigh_converged_each']}")
        for it, v in enumerate(obj):
            tail = f", flips per round {flips[it]}, min margin {margins[it]:.3e}" if it < len(flips) else " (the codes returned)"
            self.logger.info(f">>>>>> objective[{it}]: {v!r}{tail}")
        if any(info):
            self.logger.warning(f">>>>>> label regression: a pivot that was not positive (solve_info {info}); W was zeroed there")
        self.last_fit = fit
        return fit

    def train(self):
        self.logger.info("Start fit.")
        self.fit()
        self.valid(0)
        self.save_model(0)
        self.logger.info(
            f">>>>>>> FINISHED >>>>>> Best epoch, I-T: {self.best_epoch_i}, mAP: {self.max_mapi2t}, T-I: {self.best_epoch_t}, mAP: {self.max_mapt2i}")
