"""Captions and images -> hash codes with a trained checkpoint, without a dataset or a trainer: the front end of retrieve.py --text /
--image and of anything else that wants to ask an index a question.

    enc = QueryEncoder("DSPH", "result/DSPH/flickr25k/64/model-99.pth", "ViT-B-32.pt", 64)
    codes = enc.encode_text(["a dog on a beach"])                 # f32 [1, 64] in {-1, 0, +1}
    idx, dist = CodeIndex.load("db.npz").search(codes, 10)
    soft = enc.encode_text(["a dog on a beach"], soft=True)      # f32 [1, 64]: the head's output before the code rule
    idx, dist, wdist = CodeIndex.load("db.npz").search_soft(soft, 10)

The model is built as its trainer's _init_model builds it (construct, load_state_dict, float(), set_gemm_dtype, eval()), with
clip.assume_frozen = True: the weights never change here, so the towers skip their per-call parameter scan.  Text goes through the
native BPE tokenizer (dataset.base.shared_tokenizer), images through the GPU transform of the evaluation sets
(dataset.gpu_transform.preprocess, train=False), the output through the method's code rule (code_rules.py): what the trainer's
get_code* writes for the same caption or picture; with soft=True through the method's soft rule instead: the real-valued output
whose sign that code is."""
import importlib

MODELS = {"DSPH": ("model.DSPH", "MDSPH"), "DCHMT": ("model.DCHMT", "MDCMHT"), "DNPH": ("model.DNPH_TOMM", "MDNPH"),
          "DNpH": ("model.DNpH_TMM", "MDNpH"), "DMsH_LN": ("model.DMsH_LN", "MDMsH_LN"), "DHaPH": ("model.DHaPH", "MDHaPH"),
          "DDBH": ("model.DDBH", "MDDBH"), "ITQ": ("model.ITQ", "MITQ"), "DCH": ("model.DCH", "MDCH"),
          "DJSRH": ("model.DJSRH", "MDJSRH"), "MSCH": ("model.MSCH", "MMSCH"),
          "CPFH": ("model.DScPH", "MDScPH"), "DWSH": ("model.DDWSH", "MDDWSH")}
REFUSED = {"MITH": "its encoders take key padding masks and the towers' token trunks (train/MITH/hash_train.py::get_code)",
           "TwDH": "it hashes into long and short codes through centre assets (train/TwDH/hash_train.py)"}


def check_method(method):
    """NotImplementedError for MITH and TwDH, ValueError for a name that is no method: by name alone, nothing is loaded."""
    if method in REFUSED:
        raise NotImplementedError(f"QueryEncoder: method {method} is not supported: {REFUSED[method]}")
    if method not in MODELS:
        raise ValueError(f"QueryEncoder: unknown method {method!r}: one of {sorted(MODELS)}")


class QueryEncoder:

    def __init__(self, method, pretrained, clip_path, output_dim, max_words=32, resolution=224, gemm_dtype="f32", device=None,
                 bpe_path=None):
        check_method(method)                                       # before anything touches the GPU
        import tempfile

        import torch

        from code_rules import code_rule, soft_rule
        self.method, self.bits = method, int(output_dim)
        self.max_words, self.resolution, self.bpe_path = int(max_words), int(resolution), bpe_path
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.rule, self.soft_rule = code_rule(method), soft_rule(method)
        state = pretrained if isinstance(pretrained, dict) else torch.load(pretrained, map_location="cpu")
        module, name = MODELS[method]
        kw = dict(outputDim=self.bits, clipPath=clip_path, saveDir=tempfile.mkdtemp(prefix="cmh_query_"), is_train=False)   # (the model's log)
        if method == "DNPH":                                       # the classifier's width is the training set's class count
            kw["num_classes"] = state["image_pre.fc.weight"].shape[0]
        self.model = getattr(importlib.import_module(module), name)(**kw).to(self.device)
        self.model.load_state_dict(state)
        self.model.float()
        self.model.clip.set_gemm_dtype(gemm_dtype)
        self.model.clip.assume_frozen = True
        self.model.eval()

    def tokenize(self, captions):
        """list of str -> int64 [n, max_words] on the CPU."""
        from dataset.base import shared_tokenizer
        if isinstance(captions, str):
            captions = [captions]
        return shared_tokenizer(self.bpe_path).encode_captions(list(captions), self.max_words)

    def encode_tokens(self, tokens, soft=False):
        import torch
        with torch.no_grad():
            return (self.soft_rule if soft else self.rule)(self.model.encode_text(tokens.to(self.device)))

    def encode_text(self, captions, soft=False):
        """list of str -> f32 [n, K] codes in {-1, 0, +1} on the GPU; soft=True: the real-valued output behind them."""
        return self.encode_tokens(self.tokenize(captions), soft)

    def encode_image(self, images, soft=False):
        """paths or uint8 [H, W, 3] arrays -> f32 [n, K] codes in {-1, 0, +1} on the GPU; soft=True: the real-valued output."""
        import numpy as np
        import torch

        from dataset.gpu_transform import RaggedImages, preprocess
        if isinstance(images, (str, bytes)) or hasattr(images, "__fspath__") or getattr(images, "ndim", 0) == 3:
            images = [images]
        arrays = []
        for im in images:
            if isinstance(im, (str, bytes)) or hasattr(im, "__fspath__"):
                from PIL import Image
                im = np.array(Image.open(im).convert("RGB"))
            arrays.append(im)
        with torch.no_grad():
            batch = RaggedImages.from_arrays(arrays).to(self.device)
            return (self.soft_rule if soft else self.rule)(self.model.encode_image(preprocess(batch, self.resolution, train=False)))
