"""Float64 reference of the 5 x 5 convolution layers: slicing and ``matmul`` only, NHWC, any device.

It never imports fmri_hip and never calls F.conv2d / F.conv_transpose2d (on the GPU those go through the vendor
convolution library).  One tap (ky, kx) of a convolution with stride s is a matrix product over a strided slice of the
zero-padded input,

    y[n, yo, xo, :] += xp[n, ky + s yo, kx + s xo, :] @ w[:, :, ky, kx].T,

and the data / weight gradients are its two adjoints.  ConvTranspose2d(k, s, p, output_padding) with a weight
[Cin][Cout][k][k] is the same three functions with the roles exchanged (``deconv_*`` below); the bias gradient is the
column sum of the cotangent.  tests/test_conv_oracle_host.py checks all of it against torch's float64 convolutions and
autograd on the CPU.

Shapes: x [N][H][W][Cin], w [Cout][Cin][k][k], y / dy [N][Ho][Wo][Cout].  ``chunk`` = images per pass (None: all):
``images_per_chunk`` picks it so that no temporary of a pass exceeds about 1 GiB; the weight gradient accumulates over
the passes in float64.
"""
import torch


def out_size(h, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1


def images_per_chunk(N, H, W, cin, Ho, Wo, cout, pad=2, limit=2 ** 30):
    """Images per pass such that the padded input, one tap's slice and the output of a pass stay under ``limit`` bytes."""
    per_image = 8 * max((H + 2 * pad) * (W + 2 * pad) * cin, Ho * Wo * cout, Ho * Wo * cin)
    return max(1, min(N, limit // per_image))


def _f64(t):
    return t.to(torch.float64)


def _padded(x, pad):
    n, h, w, c = x.shape
    xp = torch.zeros(n, h + 2 * pad, w + 2 * pad, c, dtype=torch.float64, device=x.device)
    xp[:, pad:pad + h, pad:pad + w] = x
    return xp


def _tap(ky, kx, stride, ho, wo):
    return (slice(None), slice(ky, ky + stride * (ho - 1) + 1, stride), slice(kx, kx + stride * (wo - 1) + 1, stride))


def _chunks(n, chunk):
    chunk = n if not chunk else max(1, int(chunk))
    return [(i, min(i + chunk, n)) for i in range(0, n, chunk)]


def conv_fwd(x, w, stride, pad, chunk=None):
    """Conv2d(k, stride, pad) without bias: [N][H][W][Cin] -> [N][Ho][Wo][Cout]."""
    n, h, wd, cin = x.shape
    cout, cin_w, k, _ = w.shape
    assert cin_w == cin
    ho, wo = out_size(h, k, stride, pad), out_size(wd, k, stride, pad)
    w = _f64(w)
    y = torch.empty(n, ho, wo, cout, dtype=torch.float64, device=x.device)
    for a, b in _chunks(n, chunk):
        xp = _padded(_f64(x[a:b]), pad)
        acc = torch.zeros((b - a) * ho * wo, cout, dtype=torch.float64, device=x.device)
        for ky in range(k):
            for kx in range(k):
                acc += torch.matmul(xp[_tap(ky, kx, stride, ho, wo)].reshape(-1, cin), w[:, :, ky, kx].t())
        y[a:b] = acc.reshape(b - a, ho, wo, cout)
    return y


def conv_dgrad(dy, w, stride, pad, H, W, chunk=None):
    """Adjoint of ``conv_fwd`` in x: [N][Ho][Wo][Cout] -> [N][H][W][Cin]."""
    n, ho, wo, cout = dy.shape
    cout_w, cin, k, _ = w.shape
    assert cout_w == cout and ho == out_size(H, k, stride, pad) and wo == out_size(W, k, stride, pad)
    w = _f64(w)
    dx = torch.empty(n, H, W, cin, dtype=torch.float64, device=dy.device)
    for a, b in _chunks(n, chunk):
        d = _f64(dy[a:b]).reshape(-1, cout)
        dxp = torch.zeros(b - a, H + 2 * pad, W + 2 * pad, cin, dtype=torch.float64, device=dy.device)
        for ky in range(k):
            for kx in range(k):
                dxp[_tap(ky, kx, stride, ho, wo)] += torch.matmul(d, w[:, :, ky, kx]).reshape(b - a, ho, wo, cin)
        dx[a:b] = dxp[:, pad:pad + H, pad:pad + W]
    return dx


def conv_wgrad(x, dy, k, stride, pad, chunk=None):
    """Adjoint of ``conv_fwd`` in w: -> [Cout][Cin][k][k]."""
    n, h, wd, cin = x.shape
    _, ho, wo, cout = dy.shape
    assert dy.shape[0] == n and ho == out_size(h, k, stride, pad) and wo == out_size(wd, k, stride, pad)
    dw = torch.zeros(cout, cin, k, k, dtype=torch.float64, device=x.device)
    for a, b in _chunks(n, chunk):
        xp = _padded(_f64(x[a:b]), pad)
        dt = _f64(dy[a:b]).reshape(-1, cout).t()
        for ky in range(k):
            for kx in range(k):
                dw[:, :, ky, kx] += torch.matmul(dt, xp[_tap(ky, kx, stride, ho, wo)].reshape(-1, cin))
    return dw


def bias_grad(dy):
    return _f64(dy).reshape(-1, dy.shape[-1]).sum(0)


# ---- ConvTranspose2d(k, stride, pad, output_padding), weight [Cin][Cout][k][k]: the convolution with x and y exchanged
def deconv_out_size(h, k, stride, pad, out_pad):
    return (h - 1) * stride - 2 * pad + k + out_pad


def deconv_fwd(x, w, stride, pad, out_pad, chunk=None):
    k = w.shape[2]
    H = deconv_out_size(x.shape[1], k, stride, pad, out_pad)
    W = deconv_out_size(x.shape[2], k, stride, pad, out_pad)
    return conv_dgrad(x, w, stride, pad, H, W, chunk)


def deconv_dgrad(dy, w, stride, pad, chunk=None):
    return conv_fwd(dy, w, stride, pad, chunk)


def deconv_wgrad(x, dy, k, stride, pad, chunk=None):
    return conv_wgrad(dy, x, k, stride, pad, chunk)
