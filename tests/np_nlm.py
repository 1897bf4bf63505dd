"""numpy statement of the non-local-means denoising (cvo_nlm_denoise, cvo_nlm_denoise_lab): OpenCV's
FastNlMeansDenoisingInvoker for 8-bit images with the squared (L2) distance, behind cv::fastNlMeansDenoising(image, image, h,
template_window, search_window) and - through `denoise_lab` - the middle of cv::fastNlMeansDenoisingColored.  This is the
definition: the CPU twin and the kernel return exactly what `denoise` returns.  Shares no code with the library.

Restated from OpenCV's published algorithm; OpenCV is not available to these tests, so parity with a given OpenCV binary is
not pinned (DESIGN.md sections 4 and 5).  Written per offset over whole planes - the patch sum of every pixel at one offset
is a box sum of the plane of squared differences, taken from its integral in 64-bit integers - and not as OpenCV's sliding
column sums; in integers the two are the same numbers.  `literal` is the same definition as four plain loops, for tiny images.

  th = template_window // 2, sh = search_window // 2, tw = 2 th + 1, sw = 2 sh + 1 (an even size grows by one), b = th + sh
  ext: the image extended by b on every side, BORDER_REFLECT_101 repeated until the index lies inside (`reflect`)
  mult = INT_MAX // (sw sw 255); shift = the smallest p with (1 << p) >= tw tw; m = (1 << shift) / (tw tw)
  weight[d] = rint(mult exp(-(d m) / hh)), ties to even, d < int(255 255 C / m + 1), hh = h h C evaluated in float32;
              entries below 0.001 mult are 0
  out[c] = min(255, (sum_o w_o ext(i + dy, j + dx)[c] + ws // 2) // ws), w_o = weight[dist_o >> shift], ws = sum_o w_o,
           dist_o = the sum over the tw x tw template and the C channels of (ext(i + ty, j + tx) - ext(i + ty + dy, j + tx + dx))^2
The centre offset has distance 0, so ws >= mult > 0; est <= INT_MAX and est + ws // 2 < 2^32 by the choice of mult: asserted."""
import numpy as np

INT_MAX = 2**31 - 1


def constants(template_window, search_window):
    th, sh = template_window // 2, search_window // 2
    tw, sw = 2 * th + 1, 2 * sh + 1
    shift = 0
    while (1 << shift) < tw * tw:
        shift += 1
    return dict(th=th, sh=sh, tw=tw, sw=sw, mult=INT_MAX // (sw * sw * 255), shift=shift, m=float(1 << shift) / (tw * tw))


def weights(h, channels, template_window=7, search_window=21):
    """-> dict(weight: int64 table, mult, shift, n_nonzero, tie: the smallest distance of a mult w from a rounding tie)."""
    k = constants(template_window, search_window)
    n = int(255 * 255 * channels / k["m"] + 1)
    hh = float(np.float32(h) * np.float32(h) * np.float32(channels))
    x = k["mult"] * np.exp(-(np.arange(n) * k["m"]) / hh)
    w = np.rint(x).astype(np.int64)
    w[w < 0.001 * k["mult"]] = 0
    nz = int(np.count_nonzero(w))
    assert np.all(w[:nz] > 0) and w[0] == k["mult"]  # the weights fall: the nonzero entries are a leading run
    return dict(weight=w, mult=k["mult"], shift=k["shift"], n_nonzero=nz, tie=float(np.abs(x - np.floor(x) - 0.5).min()))


def reflect(p, n):
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * (n - 1) - p
    return p


def extend(img, b):
    """(rows + 2 b, cols + 2 b, C) int64"""
    R, W, _ = img.shape
    ri = np.array([reflect(i - b, R) for i in range(R + 2 * b)])
    ci = np.array([reflect(j - b, W) for j in range(W + 2 * b)])
    return img[ri][:, ci].astype(np.int64)


def _as3(img):
    img = np.asarray(img, np.uint8)
    return img.reshape(img.shape[0], img.shape[1], -1)


def denoise(image, h=10, template_window=7, search_window=21):
    """The denoised image, of the input's shape: (rows, cols) or (rows, cols, C) uint8, C = 1, 2 or 3."""
    img = _as3(image)
    R, W, C = img.shape
    t = weights(h, C, template_window, search_window)
    k = constants(template_window, search_window)
    th, sh, tw = k["th"], k["sh"], k["tw"]
    ext = extend(img, th + sh)
    est, ws = np.zeros((R, W, C), np.int64), np.zeros((R, W), np.int64)
    a = ext[sh:sh + R + 2 * th, sh:sh + W + 2 * th]
    for dy in range(-sh, sh + 1):
        for dx in range(-sh, sh + 1):
            q = ext[sh + dy:sh + dy + R + 2 * th, sh + dx:sh + dx + W + 2 * th]
            I = np.zeros((R + 2 * th + 1, W + 2 * th + 1), np.int64)
            I[1:, 1:] = ((a - q) ** 2).sum(2).cumsum(0).cumsum(1)
            dist = I[tw:, tw:] - I[:-tw, tw:] - I[tw:, :-tw] + I[:-tw, :-tw]
            w = t["weight"][dist >> t["shift"]]
            ws += w
            est += w[..., None] * q[th:th + R, th:th + W]
    assert ws.min() >= t["mult"] and est.max() <= INT_MAX and est.max() + ws.max() // 2 < 2**32
    out = (est + (ws // 2)[..., None]) // ws[..., None]
    return np.minimum(out, 255).astype(np.uint8).reshape(np.shape(image))


def literal(image, h=10, template_window=7, search_window=21):
    """The same definition, pixel by pixel and offset by offset, python integers throughout: for images of a few pixels."""
    img = _as3(image)
    R, W, C = img.shape
    t = weights(h, C, template_window, search_window)
    k = constants(template_window, search_window)
    th, sh = k["th"], k["sh"]

    def px(y, x, c):
        return int(img[reflect(y, R), reflect(x, W), c])

    out = np.zeros((R, W, C), np.uint8)
    for i in range(R):
        for j in range(W):
            ws, est = 0, [0] * C
            for dy in range(-sh, sh + 1):
                for dx in range(-sh, sh + 1):
                    dist = sum((px(i + ty, j + tx, c) - px(i + ty + dy, j + tx + dx, c)) ** 2
                               for ty in range(-th, th + 1) for tx in range(-th, th + 1) for c in range(C))
                    w = int(t["weight"][dist >> t["shift"]])
                    ws += w
                    for c in range(C):
                        est[c] += w * px(i + dy, j + dx, c)
            for c in range(C):
                out[i, j, c] = min(255, (est[c] + ws // 2) // ws)
    return out.reshape(np.shape(image))


def denoise_lab(lab, h=10, h_color=10, template_window=7, search_window=21):
    """The middle of fastNlMeansDenoisingColored: L as a 1-channel image with h, ab as one 2-channel image with h_color."""
    lab = np.asarray(lab, np.uint8)
    out = np.empty_like(lab)
    out[..., 0] = denoise(lab[..., 0], h, template_window, search_window)
    out[..., 1:] = denoise(lab[..., 1:], h_color, template_window, search_window)
    return out
