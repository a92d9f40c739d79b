"""Torch restatement of the two Grad-CAM kernels (csrc/gradcam.hip): the channel weights, and raw map / normalise / upsample.
Every function takes a dtype: torch.float64 is the yardstick the kernels are held to, torch.float32 on the same inputs shows
how much plain float arithmetic moves the result (the tolerance of tests/test_gpu_gradcam.py is a multiple of that).  The
formulas are the reference's (interpretability/gradcam_atualizado.py:218-220, 245-255, 284-304), written for R rows that
share N images through row_image."""
import torch
import torch.nn.functional as F

VARIANTS = 5      # metadata variants per image of the end-to-end cases


def det_rows(n_images, hw, variants=VARIANTS):
    """The end-to-end inputs: the images of det_inputs(n_images, hw, 20, 6) (what test_gpu_model.py's Grad-CAM tests feed) and
    `variants` metadata rows per image, variant v of image n being row n of det_inputs(..., salt=v)'s metadata; image-major
    [n_images * variants, 20]."""
    from oracle.detinit import det_inputs
    img = det_inputs(n_images, hw, 20, 6)[0]
    metas = torch.stack([det_inputs(n_images, hw, 20, 6, salt=v)[1] for v in range(variants)], dim=1)
    return img, metas.reshape(n_images * variants, 20).contiguous()


def clamped(row_image, n_images):
    return row_image.long().clamp(0, n_images - 1)


def gradients(acts, jac, dfeat, row_image, dtype):
    """(activations of every row [R, C, fh, fw], gradient of every row [R, C, fh, fw])"""
    n = clamped(row_image, acts.shape[0])
    a = acts.to(dtype)[n]
    if dfeat is None:
        return a, jac.to(dtype)
    return a, jac.to(dtype)[n] * dfeat.to(dtype)[:, :, None, None]


def plusplus_denominator(acts, jac, dfeat, row_image, dtype):
    """(2 g^2 + sum(A g^3) + 1e-8, 2 g^2 + |sum(A g^3)| + 1e-8), both [R, C, fh, fw]: the second is what the first would be
    without cancellation"""
    a, g = gradients(acts, jac, dfeat, row_image, dtype)
    t = (a * g ** 3).sum(dim=(2, 3), keepdim=True)
    return 2 * g ** 2 + t + 1e-8, 2 * g ** 2 + t.abs() + 1e-8


def weights(acts, jac, dfeat, row_image, mode, dtype):
    """[R, C]; mode 0 Grad-CAM, mode 1 Grad-CAM++"""
    a, g = gradients(acts, jac, dfeat, row_image, dtype)
    if mode == 0:
        return g.mean(dim=(2, 3))
    g2, g3 = g ** 2, g ** 3
    alpha = g2 / (2 * g2 + (a * g3).sum(dim=(2, 3), keepdim=True) + 1e-8)
    return (alpha * torch.relu(g)).sum(dim=(2, 3))


def raw_map(acts, w, row_image, dtype):
    """[R, fh, fw]"""
    a = acts.to(dtype)[clamped(row_image, acts.shape[0])]
    return (w.to(dtype)[:, :, None, None] * a).sum(dim=1)


def normalise(raw):
    """the reference's _normalize on every row of [R, fh, fw] separately"""
    x = torch.relu(raw)
    mn, mx = x.amin(dim=(1, 2), keepdim=True), x.amax(dim=(1, 2), keepdim=True)
    return (x - mn) / (mx - mn + 1e-8)


def cam(raw, size, dtype):
    """[R, H, W]: normalise, THEN upsample"""
    x = normalise(raw.to(dtype))
    return F.interpolate(x[:, None], size=tuple(size), mode="bilinear", align_corners=False)[:, 0]


def cam_upsample_first(raw, size, dtype):
    """the other order (Score-CAM's): upsample, then normalise -- what the kernels must NOT compute"""
    up = F.interpolate(raw.to(dtype)[:, None], size=tuple(size), mode="bilinear", align_corners=False)[:, 0]
    return normalise(up)


def explain(acts, jac, dfeat, row_image, mode, size, dtype):
    """(weights, raw, cam) in one go"""
    w = weights(acts, jac, dfeat, row_image, mode, dtype)
    raw = raw_map(acts, w, row_image, dtype)
    return w, raw, cam(raw, size, dtype)
