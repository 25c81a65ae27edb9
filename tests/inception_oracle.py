"""CPU twin of sgam_neurips22_amd/fid.py for the tests: the FID InceptionV3 in plain torch (NCHW, BatchNorm unfolded, runnable
in fp32 and fp64), synthetic weights under torchvision's `Inception3(num_classes=1008, aux_logits=False)` key names, and numpy
restatements of the activation statistics and of both Fréchet-distance routes.

The network is written from the layer table of the feature's specification plus the three pooling changes
of the FID variant: the `branch_pool` average of the A / C blocks and of Mixed_7b excludes the padding from its divisor, and
Mixed_7c pools with a 3 x 3 / stride 1 / padding 1 MAX.  The real checkpoint is not available to the tests: every comparison is
on `synthetic_state_dict` weights."""
import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-3
BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3}


def _c(name, cin, cout, k=1, s=1, p=0):
    k = (k, k) if isinstance(k, int) else k
    p = (p, p) if isinstance(p, int) else p
    return (name, cin, cout, k, s, p)


def block_a(name, cin, pf):
    return [_c(f"{name}.branch1x1", cin, 64),
            _c(f"{name}.branch5x5_1", cin, 48), _c(f"{name}.branch5x5_2", 48, 64, 5, 1, 2),
            _c(f"{name}.branch3x3dbl_1", cin, 64), _c(f"{name}.branch3x3dbl_2", 64, 96, 3, 1, 1),
            _c(f"{name}.branch3x3dbl_3", 96, 96, 3, 1, 1),
            _c(f"{name}.branch_pool", cin, pf)]


def block_b(name, cin):
    return [_c(f"{name}.branch3x3", cin, 384, 3, 2),
            _c(f"{name}.branch3x3dbl_1", cin, 64), _c(f"{name}.branch3x3dbl_2", 64, 96, 3, 1, 1),
            _c(f"{name}.branch3x3dbl_3", 96, 96, 3, 2)]


def block_c(name, cin, c7):
    return [_c(f"{name}.branch1x1", cin, 192),
            _c(f"{name}.branch7x7_1", cin, c7), _c(f"{name}.branch7x7_2", c7, c7, (1, 7), 1, (0, 3)),
            _c(f"{name}.branch7x7_3", c7, 192, (7, 1), 1, (3, 0)),
            _c(f"{name}.branch7x7dbl_1", cin, c7), _c(f"{name}.branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0)),
            _c(f"{name}.branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3)), _c(f"{name}.branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0)),
            _c(f"{name}.branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3)),
            _c(f"{name}.branch_pool", cin, 192)]


def block_d(name, cin):
    return [_c(f"{name}.branch3x3_1", cin, 192), _c(f"{name}.branch3x3_2", 192, 320, 3, 2),
            _c(f"{name}.branch7x7x3_1", cin, 192), _c(f"{name}.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3)),
            _c(f"{name}.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0)), _c(f"{name}.branch7x7x3_4", 192, 192, 3, 2)]


def block_e(name, cin):
    return [_c(f"{name}.branch1x1", cin, 320),
            _c(f"{name}.branch3x3_1", cin, 384), _c(f"{name}.branch3x3_2a", 384, 384, (1, 3), 1, (0, 1)),
            _c(f"{name}.branch3x3_2b", 384, 384, (3, 1), 1, (1, 0)),
            _c(f"{name}.branch3x3dbl_1", cin, 448), _c(f"{name}.branch3x3dbl_2", 448, 384, 3, 1, 1),
            _c(f"{name}.branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1)), _c(f"{name}.branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0)),
            _c(f"{name}.branch_pool", cin, 192)]


STEM = [_c("Conv2d_1a_3x3", 3, 32, 3, 2), _c("Conv2d_2a_3x3", 32, 32, 3), _c("Conv2d_2b_3x3", 32, 64, 3, 1, 1),
        _c("Conv2d_3b_1x1", 64, 80), _c("Conv2d_4a_3x3", 80, 192, 3)]
BLOCKS = [("A", "Mixed_5b", (192, 32)), ("A", "Mixed_5c", (256, 64)), ("A", "Mixed_5d", (288, 64)),
          ("B", "Mixed_6a", (288,)),
          ("C", "Mixed_6b", (768, 128)), ("C", "Mixed_6c", (768, 160)), ("C", "Mixed_6d", (768, 160)), ("C", "Mixed_6e", (768, 192)),
          ("D", "Mixed_7a", (768,)),
          ("E", "Mixed_7b", (1280,)), ("E", "Mixed_7c", (2048,))]
_BLOCK_CONVS = {"A": block_a, "B": block_b, "C": block_c, "D": block_d, "E": block_e}


def conv_table():
    """every conv of the network in state_dict order: (name, cin, cout, (kh, kw), stride, (ph, pw))"""
    out = list(STEM)
    for kind, name, args in BLOCKS:
        out += _BLOCK_CONVS[kind](name, *args)
    return out


def state_dict_shapes():
    """key -> shape, as torchvision's Inception3(num_classes=1008, aux_logits=False).state_dict() lists them"""
    shapes = {}
    for name, cin, cout, k, _, _ in conv_table():
        shapes[f"{name}.conv.weight"] = (cout, cin, k[0], k[1])
        for s in ("weight", "bias", "running_mean", "running_var"):
            shapes[f"{name}.bn.{s}"] = (cout,)
        shapes[f"{name}.bn.num_batches_tracked"] = ()
    shapes["fc.weight"] = (1008, 2048)
    shapes["fc.bias"] = (1008,)
    return shapes


def synthetic_state_dict(seed=0):
    """fp32 weights that keep the activations O(1) through all 94 convs: conv weights N(0, 2 / fan_in) (a ReLU output of a unit
    normal has second moment 1/2, so the pre-activation keeps unit variance), BatchNorm close to the identity with a small
    positive shift, so that about half of every layer is positive."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shape in state_dict_shapes().items():
        if key.endswith("conv.weight"):
            fan_in = shape[1] * shape[2] * shape[3]
            sd[key] = torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5
        elif key.endswith("bn.weight"):
            sd[key] = 0.9 + 0.2 * torch.rand(shape, generator=g)
        elif key.endswith("bn.bias"):
            sd[key] = 0.05 + 0.1 * torch.randn(shape, generator=g)
        elif key.endswith("running_mean"):
            sd[key] = 0.1 * torch.randn(shape, generator=g)
        elif key.endswith("running_var"):
            sd[key] = 0.8 + 0.4 * torch.rand(shape, generator=g)
        elif key.endswith("num_batches_tracked"):
            sd[key] = torch.tensor(1, dtype=torch.int64)
        elif key == "fc.weight":
            sd[key] = torch.randn(shape, generator=g) * (1.0 / shape[1]) ** 0.5
        else:
            sd[key] = torch.zeros(shape)
    return sd


# ---- the pieces -------------------------------------------------------------------------------------------------------------
def preprocess(x, resize_input=True, normalize_input=True):
    """x (B,3,H,W) in [0,1] (uint8 frames: x / 255 first) -> the network's input, in x's dtype.  Bilinear, align_corners=False,
    PyTorch's index rule written out so that it runs in fp64 with the SAME fp32 scale and source coordinates as the kernel."""
    if resize_input:
        x = bilinear(x, 299, 299)
    return 2 * x - 1 if normalize_input else x


def _axis(n_in, n_out):
    scale = np.float32(n_in) / np.float32(n_out)
    src = np.maximum((np.arange(n_out, dtype=np.float32) + np.float32(0.5)) * scale - np.float32(0.5), np.float32(0)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(np.float32)            # fp32, as the kernel forms it
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(l1.astype(np.float64))


def bilinear(x, Ho, Wo):
    y0, y1, h1 = _axis(x.shape[2], Ho)
    x0, x1, w1 = _axis(x.shape[3], Wo)
    h1, w1 = h1.to(x.dtype)[:, None], w1.to(x.dtype)[None, :]
    h0, w0 = 1 - h1, 1 - w1
    r0, r1 = x[:, :, y0], x[:, :, y1]
    return h0 * (w0 * r0[..., x0] + w1 * r0[..., x1]) + h1 * (w0 * r1[..., x0] + w1 * r1[..., x1])


def maxpool_s2(x):
    return F.max_pool2d(x, 3, 2)


def maxpool_s1p1(x):
    return F.max_pool2d(x, 3, 1, 1)


def avgpool_nopad(x):
    """3 x 3 / stride 1 / padding 1 average over the taps inside the map: the valid taps summed in (ky, kx) order, divided by
    their count (written out, so that the order is the kernel's)"""
    B, C, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    ones = F.pad(torch.ones((1, 1, H, W), dtype=x.dtype), (1, 1, 1, 1))
    s, n = torch.zeros_like(x), torch.zeros((1, 1, H, W), dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            s = s + xp[:, :, ky:ky + H, kx:kx + W]
            n = n + ones[:, :, ky:ky + H, kx:kx + W]
    return s / n


def conv_bn_relu(sd, name, x, stride=1, padding=(0, 0)):
    t = lambda k: sd[f"{name}.{k}"].to(x.dtype)      # noqa: E731
    y = F.conv2d(x, t("conv.weight"), None, stride, padding)
    y = F.batch_norm(y, t("bn.running_mean"), t("bn.running_var"), t("bn.weight"), t("bn.bias"), False, 0.0, BN_EPS)
    return F.relu(y)


def _run(sd, convs, x):
    for name, _, _, _, s, p in convs:
        x = conv_bn_relu(sd, name, x, s, p)
    return x


def run_block(sd, kind, name, args, x):
    c = {row[0][len(name) + 1:]: row for row in _BLOCK_CONVS[kind](name, *args)}
    r = lambda keys, v: _run(sd, [c[k] for k in keys], v)     # noqa: E731
    if kind == "A":
        return torch.cat([r(["branch1x1"], x), r(["branch5x5_1", "branch5x5_2"], x),
                          r(["branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"], x), r(["branch_pool"], avgpool_nopad(x))], 1)
    if kind == "B":
        return torch.cat([r(["branch3x3"], x), r(["branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"], x), maxpool_s2(x)], 1)
    if kind == "C":
        return torch.cat([r(["branch1x1"], x), r(["branch7x7_1", "branch7x7_2", "branch7x7_3"], x),
                          r([f"branch7x7dbl_{i}" for i in range(1, 6)], x), r(["branch_pool"], avgpool_nopad(x))], 1)
    if kind == "D":
        return torch.cat([r(["branch3x3_1", "branch3x3_2"], x), r([f"branch7x7x3_{i}" for i in range(1, 5)], x), maxpool_s2(x)], 1)
    b3 = r(["branch3x3_1"], x)
    bd = r(["branch3x3dbl_1", "branch3x3dbl_2"], x)
    pool = maxpool_s1p1(x) if name == "Mixed_7c" else avgpool_nopad(x)
    return torch.cat([r(["branch1x1"], x), r(["branch3x3_2a"], b3), r(["branch3x3_2b"], b3),
                      r(["branch3x3dbl_3a"], bd), r(["branch3x3dbl_3b"], bd), r(["branch_pool"], pool)], 1)


def forward(sd, x, output_blocks=(3,), resize_input=True, normalize_input=True):
    """x (B,3,H,W) in [0,1], fp32 or fp64 -> list of the selected block outputs (NCHW), ascending"""
    x = preprocess(x, resize_input, normalize_input)
    outs, last = [], max(output_blocks)
    x = maxpool_s2(_run(sd, STEM[:3], x))
    if 0 in output_blocks:
        outs.append(x)
    if last >= 1:
        x = maxpool_s2(_run(sd, STEM[3:], x))
        if 1 in output_blocks:
            outs.append(x)
    if last >= 2:
        for kind, name, args in BLOCKS[:8]:
            x = run_block(sd, kind, name, args, x)
        if 2 in output_blocks:
            outs.append(x)
    if last >= 3:
        for kind, name, args in BLOCKS[8:]:
            x = run_block(sd, kind, name, args, x)
        if 3 in output_blocks:
            outs.append(x.mean(dim=(2, 3), keepdim=True))
    return outs


def features(sd, x, dims=2048, dtype=torch.float64, resize_input=True):
    """(B,3,H,W) in [0,1] -> (B, dims) pooled features, as fid_score.get_activations forms them"""
    with torch.no_grad():
        y = forward(sd, x.to(dtype), (BLOCK_INDEX_BY_DIM[dims],), resize_input)[0]
    return y.mean(dim=(2, 3)).numpy()


# ---- statistics and distances in numpy fp64 ---------------------------------------------------------------------------------
def statistics(act):
    act = np.asarray(act, np.float64)
    return act.mean(axis=0), np.cov(act, rowvar=False)


def frechet_sqrtm(mu1, s1, mu2, s2, eps=1e-6):
    """|mu1 - mu2|^2 + tr(s1) + tr(s2) - 2 tr sqrtm(s1 s2), the matrix-square-root route (scipy), with the usual repair of a
    singular product: eps on both diagonals and a second square root"""
    from scipy import linalg
    diff = mu1 - mu2
    root = linalg.sqrtm(s1 @ s2)
    if not np.isfinite(root).all():
        off = np.eye(s1.shape[0]) * eps
        root = linalg.sqrtm((s1 + off) @ (s2 + off))
    return float(diff @ diff + np.trace(s1) + np.trace(s2) - 2.0 * np.trace(np.real(root)))


def frechet_eigh(mu1, s1, mu2, s2):
    """the same quantity through symmetric factorizations only: tr sqrt(s1 s2) = sum sqrt(eig(s1^1/2 s2 s1^1/2))"""
    w, v = np.linalg.eigh(s1)
    h = (v * np.sqrt(np.clip(w, 0.0, None))) @ v.T
    ev = np.linalg.eigvalsh(h @ s2 @ h)
    diff = mu1 - mu2
    return float(diff @ diff + np.trace(s1) + np.trace(s2) - 2.0 * np.sqrt(np.clip(ev, 0.0, None)).sum())


def frechet_lowrank(f1, f2):
    """from the feature sets themselves: with A_i = centred features / sqrt(N_i - 1), tr sqrt(s1 s2) is the sum of the singular
    values of A2 A1^T and tr(s_i) = |A_i|_F^2"""
    f1, f2 = np.asarray(f1, np.float64), np.asarray(f2, np.float64)
    a1 = (f1 - f1.mean(0)) / np.sqrt(f1.shape[0] - 1)
    a2 = (f2 - f2.mean(0)) / np.sqrt(f2.shape[0] - 1)
    diff = f1.mean(0) - f2.mean(0)
    return float(diff @ diff + (a1 * a1).sum() + (a2 * a2).sum() - 2.0 * np.linalg.svd(a2 @ a1.T, compute_uv=False).sum())
