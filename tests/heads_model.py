"""TEST INFRASTRUCTURE for the segmentation heads and the chal_* projections: `decoder_model.DecoderStandIn` with `head_l`, `head_r` and
`chal_0 .. chal_4` in the reference's layout (models/SemStereo.py:200-201, 213-217) instead of single layers.  `head_twins=True`
builds them from this repo's twins (modules.segmenthead / ChalProjection); `head_twins=False` from plain containers with the
reference's attribute layout and state_dict keys, which is what `accelerate(model, heads=True)` adopts on a box where the reference
itself is absent."""
import torch.nn as nn
import torch.nn.functional as F

import decoder_model

CHAL_IN = (128, 256, 512, 768, 512)


class PlainHead(nn.Module):
    """attribute layout of the reference's segmenthead: `conv1` with .conv, .bn, .use_bn, .relu; `conv2`; `scale_factor`"""

    def __init__(self, M, inplanes=128, interplanes=32, outplanes=6, scale_factor=2):
        super().__init__()
        self.conv1 = M.BasicConv(inplanes, interplanes, kernel_size=3, padding=1)
        self.conv2 = nn.Conv2d(interplanes, outplanes, 1)
        self.scale_factor = scale_factor

    def forward(self, x):
        x = F.relu(self.conv1.bn(self.conv1.conv(x)))
        out = self.conv2(x)
        if self.scale_factor is not None:
            out = F.interpolate(out, size=[x.shape[-2] * self.scale_factor, x.shape[-1] * self.scale_factor], mode="bilinear",
                                align_corners=False)
        return out


class PreActHead(nn.Module):
    """attribute layout of the WHU variant's pre-activation head (models/submodule_.py:63-86): bn1, conv1, bn2, relu, conv2"""

    def __init__(self, inplanes=128, interplanes=32, outplanes=6, scale_factor=2):
        super().__init__()
        self.bn1 = nn.BatchNorm2d(inplanes)
        self.conv1 = nn.Conv2d(inplanes, interplanes, kernel_size=3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(interplanes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(interplanes, outplanes, kernel_size=1, padding=0, bias=True)
        self.scale_factor = scale_factor

    def forward(self, x):
        x = self.conv1(self.relu(self.bn1(x)))
        out = self.conv2(self.relu(self.bn2(x)))
        return F.interpolate(out, size=[x.shape[-2] * self.scale_factor, x.shape[-1] * self.scale_factor], mode="bilinear",
                             align_corners=False)


class HeadsStandIn(decoder_model.DecoderStandIn):
    def __init__(self, maxdisp, M, twins=True, head_twins=False, **kw):
        super().__init__(maxdisp, M, twins=twins, **kw)
        if head_twins:
            self.head_l, self.head_r = M.segmenthead(128, 32, 6, 2), M.segmenthead(128, 32, 6, 2)
        else:
            self.head_l, self.head_r = PlainHead(M), PlainHead(M)
        for i, (ci, co) in enumerate(zip(CHAL_IN, self.chans2)):
            setattr(self, f"chal_{i}", M.ChalProjection(ci, co) if head_twins else nn.Sequential(nn.Conv2d(ci, co, 1), nn.BatchNorm2d(co)))
