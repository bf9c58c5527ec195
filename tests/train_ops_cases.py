"""Inputs that steer the fp32 per-channel training kernels (csrc/train_ops.hip: the BatchNorm statistics / apply / backward kernels in their
scalar and 16-byte forms, ss_channel_sum_fwd, the depthwise `patch` weight gradient, the gate's logits gradient; csrc/conv3d_wgrad.hip:
conv_wgrad_k1) onto each of their paths, the host rules that choose a path restated in Python, and the float64 references --
importable without a GPU (tests/test_train_ops_cases.py checks all of it on the CPU, tests/test_train_ops_paths_gpu.py runs the kernels).

Which form a call gets:
  * reduce_grid(N): one chunk (workgroup) per 16 384 elements of a channel row, `per_block` rounded up to whole 16-byte words;
  * the reduce kernel takes its 16-byte loop where N % 4 == 0, per_block % 4 == 0 and the tensors IT reads (x; in the backward grad_y, x
    and y) are 16-byte aligned -- a NULL y counts as aligned;
  * the apply kernels take theirs where vec4_ok holds: N % 4 == 0 and every tensor of the pass aligned (forward: x, residual, y;
    backward: grad_y, x, y, grad_x, grad_residual);
  * so one call can mix the forms: a misaligned residual leaves the statistics on the vector loop and sends the apply pass to the scalar
    kernel, a misaligned grad_x does the same to the backward.
The apply kernels' grid-stride loop takes a second iteration only above 65535 x 4096 elements per channel (apply_grid's cap): 1 GiB of
fp32 per channel and batch element.  That is not tested."""
import torch
import torch.nn.functional as F

import train_calls as TC
from oracle import detdata as dd

#: elements of a channel row per reduction chunk (reduce_grid), threads per workgroup, elements per 16-byte word
REDUCE_CHUNK, THREADS, WORD = 16384, 256, 4


# ---- the host rules, restated ----------------------------------------------------------------------------------------------------------

def _cdiv(a, b):
    return -(-a // b)


def reduce_grid(N):
    """-> (chunks, per_block) of train_ops.hip's reduce_grid."""
    blocks = min((N + REDUCE_CHUNK - 1) // REDUCE_CHUNK, 65535)
    per_block = (N + blocks - 1) // blocks
    per_block = (per_block + 3) // 4 * 4
    return (N + per_block - 1) // per_block, per_block


def _aligned(*addresses):
    bits = 0
    for a in addresses:
        bits |= int(a or 0)                       # (None / 0: a NULL pointer has no bits)
    return bits & 15 == 0


def vec4_ok(N, *addresses):
    """The apply kernels' rule: 16 bytes per lane where N % 4 == 0 and every tensor of the pass is 16-byte aligned."""
    return N % 4 == 0 and _aligned(*addresses)


def reduce_is_vector(N, *addresses):
    """channel_reduce_kernel's own rule, on the tensors the reduce pass reads."""
    _, per_block = reduce_grid(N)
    return N % 4 == 0 and per_block % 4 == 0 and _aligned(*addresses)


def apply_grid(N):
    return min(max(1, (N + 4095) // 4096), 65535)


def chunk_lengths(N):
    gx, per_block = reduce_grid(N)
    return [min(per_block, N - i * per_block) for i in range(gx)]


def depthwise_rows(D, H):
    """-> (rows_per_block, blocks, rows of the last block) of ss_depthwise_patch_wgrad_fwd."""
    rows = D * H
    rpb = max(1, (rows + 63) // 64)
    blocks = (rows + rpb - 1) // rpb
    return rpb, blocks, rows - (blocks - 1) * rpb


def k1_wgrad_plan(B, Cin, Cout, npos, grad_out_address=0, in_address=0):
    """ss_conv_k1_wgrad_fwd's launch: tiles, splits, pos_per_wg, gx, and per workgroup along x whether conv_wgrad_k1 takes its 16-byte
    staging loop (npos % 4 == 0, the workgroup's first position % 4 == 0, both operands aligned) and how many positions it owns."""
    ci_tiles = (Cin + 31) // 32
    tiles = ci_tiles * ((Cout + 31) // 32)
    splits = max(1, 2048 // (tiles * B))
    pos_per_wg = max(128, _cdiv(_cdiv(npos, splits), 128) * 128)
    gx = _cdiv(npos, pos_per_wg)
    vec = [npos % 4 == 0 and (i * pos_per_wg) % 4 == 0 and _aligned(grad_out_address, in_address) for i in range(gx)]
    return {"ci_tiles": ci_tiles, "tiles": tiles, "splits": splits, "pos_per_wg": pos_per_wg, "gx": gx, "vec": vec,
            "positions": [min(pos_per_wg, npos - i * pos_per_wg) for i in range(gx)]}


# ---- BatchNorm cases ---------------------------------------------------------------------------------------------------------------------

#: tensors of a forward / backward pass that a case may put one float into its buffer
FWD_TENSORS, BWD_TENSORS = ("x", "residual", "y"), ("grad_y", "x", "y", "grad_x", "grad_residual")
ALL_TENSORS = ("x", "residual", "y", "grad_y", "grad_x", "grad_residual")

#: name -> ((B, C, spatial), tensors stored one float off a 16-byte boundary, the forms the case is named for:
#: (forward statistics, forward apply, backward sums, backward apply), chunks)
BN_CASES = {
    "scalar_105": ((2, 3, (3, 5, 7)), (), ("scalar", "scalar", "scalar", "scalar"), 1),
    "vector_4": ((1, 5, (2, 2)), (), ("vector", "vector", "vector", "vector"), 1),
    "vector_1280": ((2, 4, (4, 16, 20)), (), ("vector", "vector", "vector", "vector"), 1),
    "vector_two_chunks_16388": ((1, 2, (4, 17, 241)), (), ("vector", "vector", "vector", "vector"), 2),
    "scalar_two_chunks_16385": ((2, 2, (5, 29, 113)), (), ("scalar", "scalar", "scalar", "scalar"), 2),
    "misaligned_1280": ((2, 4, (4, 16, 20)), ALL_TENSORS, ("scalar", "scalar", "scalar", "scalar"), 1),
    "misaligned_16388": ((1, 2, (4, 17, 241)), ALL_TENSORS, ("scalar", "scalar", "scalar", "scalar"), 2),
    # only the residual (forward) and only grad_x (backward) off the boundary: vector sums, scalar apply.  Without a residual the forward
    # of this case is vector_1280's.
    "mixed_1280": ((2, 4, (4, 16, 20)), ("residual", "grad_x"), ("vector", "scalar", "vector", "scalar"), 1),
}
#: the cases of the range tests and of ss_channel_sum_fwd
RANGE_CASES = ("scalar_105", "vector_1280", "vector_two_chunks_16388", "misaligned_1280")
CHANNEL_SUM_CASES = ("scalar_105", "vector_two_chunks_16388", "scalar_two_chunks_16385", "misaligned_1280", "misaligned_16388")
EPS = 1e-5


def bn_shape(name):
    (B, C, spatial), _, _, _ = BN_CASES[name]
    N = 1
    for s in spatial:
        N *= s
    return B, C, spatial, N


def _salt(name):
    return 2000 + 20 * sorted(BN_CASES).index(name)


def bn_case(name):
    """-> dict of CPU fp32 tensors: x (mean 0.3, std 2, as test_training_kernels_vs_float64_autograd), weight, bias, residual, grad_y,
    and running statistics for the eval forms (mean, var)."""
    B, C, spatial, _ = bn_shape(name)
    s, shape = _salt(name), (B, C) + tuple(spatial)
    return {"x": dd.t_normalish(shape, s) * 2 + 0.3, "weight": dd.t_uniform((C,), s + 1, 0.5, 1.5), "bias": dd.t_uniform((C,), s + 2, -0.3, 0.3),
            "residual": dd.t_normalish(shape, s + 3), "grad_y": dd.t_normalish(shape, s + 4),
            "run_mean": dd.t_uniform((C,), s + 5, -0.4, 0.4), "run_var": dd.t_uniform((C,), s + 6, 0.5, 2.0)}


def offsets(name, residual=True):
    """{tensor: 0 or 1}: floats between the start of a 16-byte aligned buffer and the tensor, per tensor of the case."""
    off = {t: int(t in BN_CASES[name][1]) for t in ALL_TENSORS}
    if not residual:
        off["residual"] = off["grad_residual"] = 0
    return off


def addresses(off, present):
    """Stand-in addresses for the restated rules: 4 * offset for a tensor that is `present`, 0 (NULL) otherwise."""
    return {t: (4 * off[t] if present.get(t, True) else 0) for t in ALL_TENSORS}


def expected_forms(N, addr):
    """(forward statistics, forward apply, backward sums, backward apply) from the restated rules on addresses {tensor: address}."""
    pick = lambda v: "vector" if v else "scalar"
    return (pick(reduce_is_vector(N, addr["x"])), pick(vec4_ok(N, *[addr[t] for t in FWD_TENSORS])),
            pick(reduce_is_vector(N, addr["grad_y"], addr["x"], addr["y"])), pick(vec4_ok(N, *[addr[t] for t in BWD_TENSORS])))


# ---- float64 (or any dtype) references ----------------------------------------------------------------------------------------------------

def bn_eval_ref(x, mean, invstd, weight, bias, relu, residual, mask=None):
    """y = (x - mean) * invstd * w + b [+ residual] [ReLU on `mask`] with the caller's statistics -> (y, pre-activation)."""
    shape = TC._cshape(x)
    z = (x - mean.reshape(shape)) * invstd.reshape(shape)
    if weight is not None:
        z = z * weight.reshape(shape)
    if bias is not None:
        z = z + bias.reshape(shape)
    if residual is not None:
        z = z + residual
    y = z
    if relu:
        y = z * ((z > 0) if mask is None else mask).to(z.dtype)
    return y, z


def bn_reference(t, dtype, relu, residual, weight, bias, batch_statistics, mask=None, stats=None):
    """Forward and backward of one configuration in `dtype` under CPU autograd on the tensors `t` of bn_case (or of a range case).
    `weight` / `bias` False: the affine term absent -- its would-be gradient (sum g' xhat / sum g') is still returned, as the kernels
    leave it in `work`.  `stats` = (mean, invstd) of the eval form (batch_statistics False), as the kernel receives them.
    -> dict: y, z (pre-activation), mean, var_unbiased (batch statistics), grad_x, grad_residual, grad_weight, grad_bias, sum_x, sum_xx."""
    x = t["x"].to(dtype).requires_grad_(True)
    C = x.shape[1]
    w = (t["weight"].to(dtype) if weight else torch.ones(C, dtype=dtype)).requires_grad_(True)
    b = (t["bias"].to(dtype) if bias else torch.zeros(C, dtype=dtype)).requires_grad_(True)
    r = t["residual"].to(dtype).requires_grad_(True) if residual else None
    m = None if mask is None else mask.to(dtype)
    out = {}
    if batch_statistics:
        y, mean, var_u, z = TC.batchnorm_ref(x, w, b, EPS, relu, r, m)
        out.update(mean=mean.detach(), var_unbiased=var_u.detach())
    else:
        y, z = bn_eval_ref(x, stats[0].to(dtype), stats[1].to(dtype), w, b, relu, r, m)
    leaves = [x, w, b] + ([r] if residual else [])
    grads = torch.autograd.grad(y, leaves, t["grad_y"].to(dtype))
    dims = [0] + list(range(2, x.dim()))
    out.update(y=y.detach(), z=z.detach(), grad_x=grads[0], grad_weight=grads[1], grad_bias=grads[2],
               grad_residual=grads[3] if residual else None, sum_x=x.detach().sum(dims), sum_xx=(x.detach() ** 2).sum(dims))
    return out


# ---- the range inputs ---------------------------------------------------------------------------------------------------------------------

RANGE_OFFSETS, RANGE_SCALES, CONSTANT_VALUE = (0.0, 10.0, 100.0, 1000.0), (1e-3, 1.0, 1e3), 1000.1


def range_channels():
    """[(off, scale)] per channel, neighbouring channels differing in both; the last channel (None) is the constant one."""
    chans = [(RANGE_OFFSETS[(i + j) % 4], RANGE_SCALES[j]) for i in range(4) for j in range(3)]
    return chans + [None]


def range_case(name):
    """The tensors of bn_case at the case's (B, spatial) with 13 channels drawn as (normal + off) * scale, one constant."""
    B, _, spatial, _ = bn_shape(name)
    chans = range_channels()
    C, s = len(chans), _salt(name) + 10
    shape = (B, C) + tuple(spatial)
    x = dd.t_normalish(shape, s).double()
    for c, oc in enumerate(chans):
        x[:, c] = CONSTANT_VALUE if oc is None else (x[:, c] + oc[0]) * oc[1]
    return {"x": x.float(), "weight": dd.t_uniform((C,), s + 1, 0.5, 1.5), "bias": dd.t_uniform((C,), s + 2, -0.3, 0.3),
            "residual": dd.t_normalish(shape, s + 3), "grad_y": dd.t_normalish(shape, s + 4)}


# ---- the neighbours -------------------------------------------------------------------------------------------------------------------

def channel_sum_case(name):
    """[B,C,N] with a mean of 0.5 std, so that the sums do not cancel."""
    B, C, _, N = bn_shape(name)
    return dd.t_normalish((B, C, N), _salt(name) + 15) + 0.5


#: (B, C, D, H, W) of ss_depthwise_patch_wgrad_fwd: 65 rows (two per block, one in the last); W = 1; H = 1; a single element; 300
#: positions in a block of one row
PATCH_CASES = {"rows_65": (2, 3, 5, 13, 7), "w1": (1, 2, 3, 4, 1), "h1": (1, 2, 3, 1, 5), "one": (1, 1, 1, 1, 1), "wide_block": (1, 2, 1, 3, 300)}


def patch_case(name):
    shape = PATCH_CASES[name]
    s = 2400 + 10 * sorted(PATCH_CASES).index(name)
    return dd.t_normalish(shape, s), dd.t_normalish(shape, s + 1)                 # grad_out, in


def patch_dead_taps(H, W):
    """[3,3] bool: taps (kh, kw) that never see the image -- kh != 1 where H == 1, kw != 1 where W == 1."""
    dead = torch.zeros((3, 3), dtype=torch.bool)
    if H == 1:
        dead[0, :] = dead[2, :] = True
    if W == 1:
        dead[:, 0] = dead[:, 2] = True
    return dead


def patch_wgrad_ref(grad_out, x):
    """[C,1,1,3,3]: autograd of the depthwise (1,3,3) convolution in the tensors' dtype."""
    C = x.shape[1]
    w = torch.zeros((C, 1, 1, 3, 3), dtype=x.dtype, requires_grad=True)
    (gw,) = torch.autograd.grad(TC.patch_ref(x, w), w, grad_out)
    return gw


#: (B, C, D, H, W): D = 1 on a plane of 257 (a partial second block); a small volume
GATE_CASES = {"d1_plane257": (1, 1, 1, 1, 257), "volume": (2, 3, 4, 5, 7)}
SATURATED_LOGITS = (30.0, -30.0, 100.0, -100.0)


def gate_case(name):
    """-> (grad_out, cv [B,C,D,H,W], logits [B,C,H,W] with the first elements of every plane at +-30 and +-100)."""
    B, C, D, H, W = GATE_CASES[name]
    s = 2500 + 10 * sorted(GATE_CASES).index(name)
    a = dd.t_normalish((B, C, H, W), s + 2).clone()
    a.reshape(B, C, H * W)[:, :, :4] = torch.tensor(SATURATED_LOGITS)
    return dd.t_normalish((B, C, D, H, W), s), dd.t_normalish((B, C, D, H, W), s + 1), a


def gate_logits_grad_ref(grad_out, cv, a):
    s = torch.sigmoid(a)
    return s * (1 - s) * (grad_out * cv).sum(dim=2)


K1_CHANNELS = ((33, 1), (3, 5), (40, 70))
#: (B, npos, operand one float off the boundary): 35 scalar; 132 vector, the second workgroup owns 4 positions; 260 at batch 3; 132 misaligned
K1_POSITIONS = {"npos35": (1, 35, None), "npos132": (2, 132, None), "npos260_b3": (3, 260, None), "npos132_misaligned": (2, 132, "in")}


def k1_case(cin, cout, name):
    B, npos, _ = K1_POSITIONS[name]
    s = 2600 + 7 * cin + cout
    return dd.t_normalish((B, cout, npos), s), dd.t_normalish((B, cin, npos), s + 1)       # grad_out, in


def k1_wgrad_ref(grad_out, x):
    return torch.einsum("bop,bip->oi", grad_out, x)
