"""DDWSH model (reference train/DDWSH/hash_train.py:28-30 builds `Baseclip` itself): Baseclip with LinearHash heads, the keys of MDSPH
(`clip.*`, `image_hash.fc.{weight,bias}`, `text_hash.fc.{weight,bias}`), so its checkpoints also load as DSPH.  The per-class boundaries
belong to the loss (train/DDWSH/loss.py) and, as in the reference, are not saved."""
import logging

from model.modelbase import Baseclip
from streams import overlapped


class MDDWSH(Baseclip):

    def __init__(self, outputDim=64, clipPath="./ViT-B-32.pt", writer=None, saveDir="./result/log",
                 logger: logging.Logger = None, is_train=True):
        super(MDDWSH, self).__init__(outputDim=outputDim, clipPath=clipPath, writer=writer,
                                     saveDir=saveDir, logger=logger, is_train=is_train)

    def forward(self, image, text):
        return overlapped(lambda: self.encode_image(image), lambda: self.encode_text(text))
