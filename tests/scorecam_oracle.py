"""numpy fp32 restatement of csrc/scorecam.hip, in the kernels' own operation order (every multiply and add rounds to fp32 on
its own, as the kernels do with contraction switched off).  tests/test_cpu_scorecam.py holds it to torch.nn.Upsample and to a
golden recorded from the reference's ScoreCAM class; tests/test_gpu_scorecam.py holds the kernels to it bit for bit."""
import numpy as np

F = np.float32


def axis_taps(n_in, n_out):
    """align_corners=False source taps of every destination index along one axis -> (i0, i1, l)."""
    scale = F(n_in) / F(n_out)
    s = (np.arange(n_out, dtype=F) + F(0.5)) * scale - F(0.5)
    s = np.where(s < 0, F(0), s).astype(F)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    lam = np.minimum(np.maximum(s - i0.astype(F), F(0)), F(1)).astype(F)
    return i0, i1, lam


def upsample(fmap, size):
    """fmap [C, fh, fw] fp32 -> [C, H, W]: torch.nn.Upsample(size, mode='bilinear') before any normalisation."""
    fmap = np.ascontiguousarray(fmap, dtype=F)
    y0, y1, ly = axis_taps(fmap.shape[1], size[0])
    x0, x1, lx = axis_taps(fmap.shape[2], size[1])
    ly, lx = ly[None, :, None], lx[None, None, :]
    f00, f01, f10, f11 = fmap[:, y0][:, :, x0], fmap[:, y0][:, :, x1], fmap[:, y1][:, :, x0], fmap[:, y1][:, :, x1]
    top = f00 + lx * (f01 - f00)          # the difference form keeps a constant channel exactly constant
    bot = f10 + lx * (f11 - f10)
    out = top + ly * (bot - top)
    assert out.dtype == F
    return out


def minmax(fmap, size):
    """-> [C, 2]: min and max of each UPSAMPLED channel."""
    up = upsample(fmap, size)
    return np.stack([up.min(axis=(1, 2)), up.max(axis=(1, 2))], axis=1).astype(F)


def cams(fmap, size):
    """-> [C, H, W]: (up - min) / (max - min), all zeros for a flat channel (ScoreCam.py:117-121)."""
    up = upsample(fmap, size)
    mn = up.min(axis=(1, 2), keepdims=True)
    rng = (up.max(axis=(1, 2), keepdims=True) - mn).astype(F)
    flat = rng == 0
    out = (up - mn) / np.where(flat, F(1), rng)
    return np.where(flat, F(0), out).astype(F)


def mask(fmap, image, c0, n, n_pad):
    """-> [n_pad, 3, H, W]: image * cam of channels c0 .. c0 + n, zero rows from n on."""
    image = np.ascontiguousarray(image, dtype=F)
    out = np.zeros((n_pad,) + image.shape, dtype=F)
    out[:n] = image[None] * cams(fmap[c0:c0 + n], image.shape[1:])[:, None]
    return out


def combine_raw(fmap, scores, size):
    """-> [H, W]: relu(sum_c scores[c] * cam_c), fp32, ascending c, product and sum rounded separately."""
    cam = cams(fmap, size)
    acc = np.zeros(size, dtype=F)
    for s, m in zip(np.asarray(scores, dtype=F), cam):
        acc = acc + s * m
    assert acc.dtype == F
    return np.where(acc < 0, F(0), acc).astype(F)


def combine(fmap, scores, size):
    """-> [H, W]: the heat map.  No zero guard on the division, as in the reference: a flat map gives NaN."""
    raw = combine_raw(fmap, scores, size)
    mn = raw.min()
    with np.errstate(invalid="ignore", divide="ignore"):
        return ((raw - mn) / (raw.max() - mn)).astype(F)
