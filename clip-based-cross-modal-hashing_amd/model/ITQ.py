"""Model of the training-free methods (LSH, PCAH, ITQ, and through model/DCH.py the supervised DCH; no upstream counterpart): Baseclip
with LinearHash heads, the keys of MDSPH (`clip.*`, `image_hash.fc.{weight,bias}`, `text_hash.fc.{weight,bias}`), so its checkpoints
also load as DSPH.  The heads are written by the fit (utils/itq.py), never trained."""
from model.modelbase import Baseclip
from streams import overlapped


class MITQ(Baseclip):

    def forward(self, image, text):
        return overlapped(lambda: self.encode_image(image), lambda: self.encode_text(text))
