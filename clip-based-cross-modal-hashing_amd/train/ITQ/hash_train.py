"""Training-free codes from a stock CLIP checkpoint (no upstream counterpart): LSH, PCAH and ITQ (Gong & Lazebnik, CVPR 2011) on
the towers' own features, and with --projection cca the paper's cross-modal variant (one projection per modality from the whitened
cross-covariance of the pairs).  train() makes one pass over the train loader without gradients, keeps the features on the GPU, fits the
two heads (utils/itq.py, csrc/itq.hip), writes them into the model, saves model-0.pth and runs the usual validation.  Labels are
read by the evaluation alone.  The checkpoint has DSPH's keys: it loads as `--method ITQ` and as `--method DSPH`."""
import os
import time

import torch

import dist_utils as du
from model.ITQ import MITQ
from train.base import TrainBase
from utils.itq import PROJECTIONS, ROTATIONS, MomentStream, fit_from_moments, load_heads
from .get_args import get_args


class ITQTrainer(TrainBase):

    def __init__(self, args, rank=0):
        args = get_args(args)
        args.rank = rank
        if args.projection not in PROJECTIONS or args.rotation not in ROTATIONS:
            raise ValueError(f"ITQ: --projection {args.projection} / --rotation {args.rotation}: one of {PROJECTIONS} and one of {ROTATIONS}")
        if args.projection == "cca" and not args.cca_reg > 0.0:
            raise ValueError(f"ITQ: --cca-reg {args.cca_reg}: the ridge must be positive")
        if du.world_size() > 1:      # before any data is touched
            raise NotImplementedError("ITQ: the fit runs on one rank (a sharded fit is not built); start it without torch.distributed.run")
        super(ITQTrainer, self).__init__(args)
        self.logger.info("dataset len: {}".format(len(self.train_loader.dataset)))
        self.run()

    def _init_model(self):
        self.logger.info("init model.")
        self.model = MITQ(outputDim=self.args.output_dim, clipPath=self.args.clip_path,
                          writer=self.writer, logger=self.logger, is_train=self.args.is_train).to(self.rank)
        if self.args.pretrained != "" and os.path.exists(self.args.pretrained):
            self.logger.info("load pretrained model.")
            self.model.load_state_dict(torch.load(self.args.pretrained, map_location=f"cuda:{self.rank}"))
        self.model.float()
        self.model.clip.set_gemm_dtype(self.args.gemm_dtype)
        self.total_time = 0

    def collect_features(self):
        """One pass over the train loader: the towers' raw features of up to --fit-num items (all of them by default), f32 on the
        GPU, and their running moments (with --projection cca the cross moments too), one batch per call."""
        limit = int(self.args.fit_num) if int(self.args.fit_num) > 0 else None
        feats_i, feats_t, moments, seen = [], [], MomentStream(cross=self.args.projection == "cca"), 0
        with torch.no_grad():
            for batch in self.train_loader:
                image, text = batch[0].to(self.rank, non_blocking=True), batch[1].to(self.rank, non_blocking=True)
                if limit is not None and seen + image.shape[0] > limit:
                    image, text = image[:limit - seen], text[:limit - seen]
                fi, ft = self.model.clip.encode_image(image).float(), self.model.clip.encode_text(text).float()
                moments.add(fi, ft)
                feats_i.append(fi)
                feats_t.append(ft)
                seen += fi.shape[0]
                if limit is not None and seen >= limit:
                    break
        return torch.cat(feats_i), torch.cat(feats_t), moments

    def fit(self):
        began = time.time()
        self.change_state(mode="valid")
        Fi, Ft, moments = self.collect_features()
        cca = self.args.projection == "cca"
        fit = fit_from_moments(Fi, Ft, moments.finish_cca() if cca else moments.finish(), self.args.output_dim, self.args.projection,
                               self.args.rotation, self.args.itq_iters, seed=self.args.seed, reg=self.args.cca_reg)
        load_heads(self.model, fit)
        self.total_time += time.time() - began
        obj = [float(v) for v in fit["objective"].cpu()]
        self.logger.info(f">>>>>> fit: {self.args.projection}+{self.args.rotation} on {Fi.shape[0]} pairs, D = {Fi.shape[1]}, "
                         f"bits = {self.args.output_dim}, scale = {float(fit['scale']):.6g}, time: {self.total_time}")
        if "evals" in fit:
            ev = fit["evals"].cpu()
            kept = float(ev[:self.args.output_dim].sum() / ev.sum())
            self.logger.info(f">>>>>> eigenvalue share kept: {kept:.6f} (Jacobi sweeps: {fit['eigh_sweeps']}, converged: {fit['eigh_converged']})")
        if cca:
            kept = fit["correlations"][:self.args.output_dim].cpu()
            self.logger.info(f">>>>>> canonical correlations kept: first {float(kept[0]):.6f}, last {float(kept[-1]):.6f}, mean {float(kept.mean()):.6f} "
                             f"(ridge {fit['reg']:g} / D; Jacobi sweeps: {fit['eigh_sweeps']}, converged: {fit['eigh_converged_each']})")
        for it, v in enumerate(obj):
            self.logger.info(f">>>>>> objective[{it}]: {v!r}")
        self.last_fit = fit
        return fit

    def train(self):
        self.logger.info("Start fit.")
        self.fit()
        self.valid(0)
        self.save_model(0)
        self.logger.info(
            f">>>>>>> FINISHED >>>>>> Best epoch, I-T: {self.best_epoch_i}, mAP: {self.max_mapi2t}, T-I: {self.best_epoch_t}, mAP: {self.max_mapt2i}")
