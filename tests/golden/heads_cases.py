"""Case table of the heads fixture (`heads.npz`), shared by `make_golden_heads.py` (which runs the REFERENCE's own segmenthead and the
`head_l`, `chal_0 .. chal_4` of its SemStereo on these inputs, in the build container only) and by the tests (which run the twins on
the same inputs, anywhere).  Weights, BatchNorm statistics and inputs are closed-form (`decoder_cases.fill`, `oracle.detdata`), so
only reference OUTPUTS are stored (`decoder_cases.record`).
"""
from oracle import detdata as dd

from golden import decoder_cases as dc

# `head_l` of SemStereo(64, False, True, True, 6) = segmenthead(128, 32, 6, 2) (models/SemStereo.py:200): name -> input shape
HEADS = {
    "full": (1, 128, 32, 48),                   # several 8 x 32 tiles
    "small": (2, 128, 5, 7),                    # smaller than a tile, odd H / W, batch 2
}
HEAD_SALT = 51
# a head the kernel is not built for (interplanes != 32): (inplanes, interplanes, outplanes, scale_factor), input shape
RAGGED = ((24, 12, 5, 2), (1, 24, 6, 9))
RAGGED_SALT = 52
# the backbone's maps after FeatUp, as chal_0 .. chal_4 see them (models/SemStereo.py:196, 213-217): channels in, channels out
CHAL_IN = (128, 256, 512, 768, 512)
CHAL_OUT = dc.CHANS2
CHAL_SALTS = {f"chal_{i}": 53 + i for i in range(5)}
RIGHT_LEVELS = (1, 2)                           # chal_1 / chal_2 also run on the right view (:264-265)


def head_input(name):
    return dd.t_normalish(HEADS[name], 1300 + sorted(HEADS).index(name))


def ragged_input():
    return dd.t_normalish(RAGGED[1], 1310)


def chal_inputs():
    """The left and the right pyramid (five maps each at 1/2 .. 1/32 of decoder_cases.PYRAMID)."""
    return dc.pyramid(CHAL_IN, 1320), dc.pyramid(CHAL_IN, 1330)


def run_all(head, ragged, chals):
    """Every case on the given modules (`head`: head_l's layout, `ragged`: segmenthead(*RAGGED[0]), `chals`: the five projections
    by name) -> {fixture key: (tensor, salt of decoder_cases.record / compare)}."""
    out = {}
    for k, name in enumerate(sorted(HEADS)):
        x = head_input(name)
        out[f"head/{name}"] = (head(x.to(_device(head))), 30 + k)
    out["head/ragged"] = (ragged(ragged_input().to(_device(ragged))), 33)
    left, right = chal_inputs()
    for i in range(5):
        mod = chals[f"chal_{i}"]
        out[f"chal/L{i}"] = (mod(left[i].to(_device(mod))), 40 + i)
    for i in RIGHT_LEVELS:
        mod = chals[f"chal_{i}"]
        out[f"chal/R{i}"] = (mod(right[i].to(_device(mod))), 50 + i)
    return out


def _device(module):
    return next(module.parameters()).device
