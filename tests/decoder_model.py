"""TEST INFRASTRUCTURE for the 2-D decoder: `standin_model.StandInSemStereo` with the REAL channel counts around its decoder
(models/SemStereo.py:62, 196-197) so that FeatUp, the spx chain and spx2 are the reference's layers.  `twins=True` builds them from
this repo's twins (modules.Conv2x / FeatUp / Spx2); `twins=False` from plain containers with the reference's attribute layout and
state_dict keys, which is what `accelerate(model, decoder=True)` adopts on a box where the reference itself is absent."""
import torch
import torch.nn as nn
import torch.nn.functional as F

import standin_model


class PlainConv2x(nn.Module):
    """attribute layout of the reference's Conv2x(deconv=True): `conv1` / `conv2` with .conv, .bn, .use_bn, .relu; `concat`, `is_3d`"""

    def __init__(self, M, cin, cout):
        super().__init__()
        self.concat, self.is_3d = True, False
        self.conv1 = M.BasicConv(cin, cout, deconv=True, kernel_size=4, stride=2, padding=1)
        self.conv2 = M.BasicConv(2 * cout, 2 * cout, kernel_size=3, stride=1, padding=1)

    def _bc(self, bc, x):
        return F.relu(bc.bn(bc.conv(x)))

    def forward(self, x, rem):
        x = self._bc(self.conv1, x)
        if x.shape != rem.shape:
            x = F.interpolate(x, size=(rem.shape[-2], rem.shape[-1]), mode="bilinear")
        return self._bc(self.conv2, torch.cat((x, rem), 1))


class PlainFeatUp(nn.Module):
    def __init__(self, M):
        super().__init__()
        self.deconv32_16, self.deconv16_8 = PlainConv2x(M, 512, 384), PlainConv2x(M, 768, 256)
        self.deconv8_4, self.deconv4_2 = PlainConv2x(M, 512, 128), PlainConv2x(M, 256, 64)

    def forward(self, featL, featR=None):
        x2, x4, x8, x16, x32 = featL
        y2, y4, y8, y16, y32 = featR
        x16, y16 = self.deconv32_16(x32, x16), self.deconv32_16(y32, y16)
        x8, y8 = self.deconv16_8(x16, x8), self.deconv16_8(y16, y8)
        x4, y4 = self.deconv8_4(x8, x4), self.deconv8_4(y8, y4)
        x2, y2 = self.deconv4_2(x4, x2), self.deconv4_2(y4, y2)
        return [x2, x4, x8, x16, x32], [y2, y4, y8, y16, y32]


class _Pyramid(nn.Module):
    """stand-in for Feature with the backbone's channel counts: 64, 128, 256, 384, 512 at 1/2 .. 1/32"""

    def __init__(self):
        super().__init__()
        self.convs = nn.ModuleList([nn.Conv2d(3, c, 3, padding=1) for c in (64, 128, 256, 384, 512)])

    def forward(self, x):
        return [conv(F.avg_pool2d(x, 2 ** (i + 1))) for i, conv in enumerate(self.convs)]


class DecoderStandIn(standin_model.StandInSemStereo):
    def __init__(self, maxdisp, M, twins=True, **kw):
        super().__init__(maxdisp, M, **kw)
        self.chans2 = [64, 128, 256, 384, 256]
        self.feature = _Pyramid()
        self.head_l, self.head_r = standin_model._Head(128, 6, 2), standin_model._Head(128, 6, 2)
        for i, (ci, co) in enumerate(zip((128, 256, 512, 768, 512), self.chans2)):
            setattr(self, f"chal_{i}", nn.Conv2d(ci, co, 1))
        if twins:
            self.feature_up = M.FeatUp()
            mk = lambda ci, co: M.Conv2x(ci, co, True)
            self.spx2 = M.Spx2(128, 6)
        else:
            self.feature_up = PlainFeatUp(M)
            mk = lambda ci, co: PlainConv2x(M, ci, co)
            self.spx2 = nn.Sequential(nn.ConvTranspose2d(128, 6, kernel_size=4, stride=2, padding=1))
        self.spx32_16, self.spx16_8, self.spx8_4, self.spx4_2 = mk(256, 384), mk(768, 256), mk(512, 128), mk(256, 64)
