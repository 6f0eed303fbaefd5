"""MSCH model: Baseclip with LinearHash heads, the keys of MDSPH (`clip.*`, `image_hash.fc.{weight,bias}`,
`text_hash.fc.{weight,bias}`), so its checkpoints also load as DSPH.  (The reference's only user of this loss, model/DPSIH.py, expects
token outputs that this CLIP does not give and is not built; the loss needs no more than two [B, K] matrices.)"""
import logging

from model.modelbase import Baseclip
from streams import overlapped


class MMSCH(Baseclip):

    def __init__(self, outputDim=64, clipPath="./ViT-B-32.pt", writer=None, saveDir="./result/log",
                 logger: logging.Logger = None, is_train=True):
        super(MMSCH, self).__init__(outputDim=outputDim, clipPath=clipPath, writer=writer,
                                    saveDir=saveDir, logger=logger, is_train=is_train)

    def forward(self, image, text):
        return overlapped(lambda: self.encode_image(image), lambda: self.encode_text(text))
