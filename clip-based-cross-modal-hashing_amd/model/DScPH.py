"""DScPH model (reference model/DScPH.py): Baseclip with LinearHash heads, the keys of MDSPH (`clip.*`,
`image_hash.fc.{weight,bias}`, `text_hash.fc.{weight,bias}`), so its checkpoints also load as DSPH.  The class proxies belong to the
loss (train/DScPH/loss.py) and, as in the reference, are not saved."""
import logging

from model.modelbase import Baseclip
from streams import overlapped


class MDScPH(Baseclip):

    def __init__(self, outputDim=64, clipPath="./ViT-B-32.pt", writer=None, saveDir="./result/log",
                 logger: logging.Logger = None, is_train=True):
        super(MDScPH, self).__init__(outputDim=outputDim, clipPath=clipPath, writer=writer,
                                     saveDir=saveDir, logger=logger, is_train=is_train)

    def forward(self, image, text):
        return overlapped(lambda: self.encode_image(image), lambda: self.encode_text(text))
