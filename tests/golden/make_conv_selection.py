"""Census of the convolution kernel selection: every answer of the host-only query entry points on a fixed problem grid.

    python tests/golden/make_conv_selection.py            # writes tests/golden/conv_selection.npz

The queries (am_conv3d_uses_k3, am_conv3d_partials_rows, am_conv3d_prenorm_supported, am_conv3d_wgrad_uses_k3,
am_conv3d_wgrad_gather_bytes) are pure host code and answer without a GPU, so the same script runs before and after a change of the
selection code; tests/test_conv_selection.py re-asks every question and requires equality.  Only the C ABI is used.

The grid = (a) every convolution launch shape of the models (engine.py: encoder blocks, densify projections, decoder blocks, the
segmentation network), forward + data gradient (every row also asks the weight-gradient questions), in all flag combinations, and
(b) a thinned product over modes, dtypes, (k, stride), batch, grid, channels, sparsity, n_active and flags.  The file stores the
answers and a digest of the problem table (the table itself is regenerated from this module), the commit it was generated at and
the CU count the library saw (`partials_rows` of the conv_k3 shapes is 8 x CUs)."""
import ctypes as C
import hashlib
import itertools
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "conv_selection.npz")

FWD, DGRAD, CT_FWD, CT_DGRAD = 0, 1, 2, 3
F32, BF16, F32S = 0, 1, 2
COLS = ("mode", "dtype", "k", "stride", "B", "Di", "Hi", "Wi", "Cin", "Do", "Ho", "Wo", "Cout", "sparse", "in_bshift", "out_bshift",
        "n_active", "accumulate", "ep", "partials", "det")
ANSWERS = ("uses_k3", "partials_rows", "prenorm_supported", "wgrad_uses_k3", "wgrad_gather_bytes")

SIZES = {"S": ([16, 32, 64, 128, 256, 256], 1, 256), "B": ([32, 64, 128, 256, 512, 512], 1, 512),
         "L": ([64 * x for x in (1, 2, 4, 8, 16, 16)], 2, 1024), "H": ([96 * x for x in (1, 2, 4, 8, 16, 16)], 3, 1536)}


def _layers(dims, width, size, B, mask_ratio, seg=False):
    """(mode, k, stride, Cin, Cout, Si, So, sparse, in_bshift, out_bshift, n_active) of every am_conv3d launch of a forward pass"""
    sp = lambda s: tuple(v >> s for v in size)
    nf = (size[0] // 16) * (size[1] // 16) * (size[2] // 16)
    na = nf if seg else B * round(nf * (1 - mask_ratio))
    out = []
    for s in range(5):                                    # encoder BasicResBlocks (stage 0's first conv is the stem kernel)
        bs, cin, c = 4 - s, dims[max(s - 1, 0)], dims[s]
        if s > 0:
            out.append((FWD, 3, 2, cin, c, sp(s - 1), sp(s), 1, bs + 1, bs, na))
            out.append((FWD, 1, 2, cin, c, sp(s - 1), sp(s), 1, bs + 1, bs, na))
        out.append((FWD, 3, 1, c, c, sp(s), sp(s), 1, bs, bs, na))
    if seg:                                               # stage 5 (stride 1 at stage 4's grid), 1x1 upsample convs, localization blocks 2C -> C
        out.append((FWD, 3, 1, dims[4], dims[5], sp(4), sp(4), 1, 0, 0, na))
        out.append((FWD, 1, 1, dims[4], dims[5], sp(4), sp(4), 1, 0, 0, na))
        for u in range(5):
            s = 4 - u
            out.append((FWD, 1, 1, dims[s + 1], dims[s], sp(min(s + 1, 4)), sp(min(s + 1, 4)), 0, 0, 0, 0))
            out.append((FWD, 3, 1, 2 * dims[s], dims[s], sp(s), sp(s), 1, 4 - s, 4 - s, na))
            out.append((FWD, 1, 1, 2 * dims[s], dims[s], sp(s), sp(s), 1, 4 - s, 4 - s, na))
            out.append((FWD, 3, 1, dims[s], dims[s], sp(s), sp(s), 1, 4 - s, 4 - s, na))
        return out
    dw = width
    for i in range(4):                                    # densify projections (coarse -> fine), dense
        if not (i == 0 and dims[4 - i] == dw):
            out.append((FWD, 1 if i == 0 else 3, 1, dims[4 - i], dw, sp(4 - i), sp(4 - i), 0, 0, 0, 0))
        dw //= 2
    for i in range(4):                                    # decoder UNetBlocks: ConvTranspose3d k4 s2, two k3 convs
        c, co = width >> i, width >> (i + 1)
        out.append((CT_FWD, 4, 2, c, c, sp(4 - i), sp(3 - i), 0, 0, 0, 0))
        out.append((FWD, 3, 1, c, c, sp(3 - i), sp(3 - i), 0, 0, 0, 0))
        out.append((FWD, 3, 1, c, co, sp(3 - i), sp(3 - i), 0, 0, 0, 0))
    c = width >> 4                                        # the teacher's last conv with a patch mask on the output (out_skip)
    out.append((FWD, 3, 1, c, c, sp(0), sp(0), -1, 0, 4, B * (nf - round(nf * (1 - mask_ratio)))))
    return out


def model_problems():
    tiny = dict(np.load(os.path.join(HERE, "forward_tiny.npz")))
    models = [(SIZES["B"], (128,) * 3, b, 0.6, False) for b in (1, 4, 16)]
    models += [(SIZES["B"], (112, 112, 128), 4, 0.6, False), (SIZES["L"], (160,) * 3, 4, 0.7, False), (SIZES["H"], (192,) * 3, 2, 0.6, False)]
    models += [(([int(v) for v in tiny["dims"]], 1, int(tiny["width"])), tuple(int(v) for v in tiny["input_size"]), int(tiny["B"]),
                float(tiny["mask_ratio"]), False)]
    models += [(SIZES["B"], (128,) * 3, 1, 0.0, True), (SIZES["S"], (32, 32, 32), 1, 0.0, True), (SIZES["S"], (32, 16, 48), 1, 0.0, True)]
    rows = []
    for (dims, _depth, width), size, B, ratio, seg in models:
        for mode, k, st, cin, cout, si, so, sparse, ibs, obs, na in _layers(dims, width, size, B, ratio, seg):
            for dt in ((BF16, F32S) if not seg else (BF16, F32)):
                for acc, ep, part, det in itertools.product((0, 1), repeat=4):
                    # sparse -1: a mask on the output only; the queries know one `sparse` flag
                    rows.append((mode, dt, k, st, B, *si, cin, *so, cout, abs(sparse), ibs, obs, na, acc, ep, part, det))
                    rows.append((mode + 1, dt, k, st, B, *so, cout, *si, cin, abs(sparse), obs, ibs, na, acc, ep, part, det))
    return rows


class _Lcg:
    """fixed pseudo-random choices (independent of any library's generator)"""

    def __init__(self, seed):
        self.s = seed

    def pick(self, seq):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        return seq[(self.s >> 33) % len(seq)]


def product_problems():
    """the product of the axes, thinned: every (mode, dtype, (k, stride), sparsity, flags) combination, each with a fixed sample of
    (B, grid, Cin, Cout, n_active, deterministic) -- three times as many for bf16, where the kernels differ"""
    ks = ((1, 1), (1, 2), (3, 1), (3, 2), (4, 2))
    grids = [(g,) * 3 for g in (4, 8, 12, 16, 20, 24, 32, 40, 64, 128)] + [(112, 112, 128)]
    chans = (8, 24, 32, 64, 96, 128, 256, 512)
    sparsity = (None, 0, 1, 2, 3, 4)
    rnd = _Lcg(20260101)
    rows = []
    for mode, dt, (k, st), obs, (acc, ep, part) in itertools.product((FWD, DGRAD, CT_FWD, CT_DGRAD), (F32, BF16, F32S), ks, sparsity,
                                                                     itertools.product((0, 1), repeat=3)):
        for _ in range(66 if dt == BF16 else 22):
            B, g, cin, cout = rnd.pick((1, 2, 255, 256)), rnd.pick(grids), rnd.pick(chans), rnd.pick(chans)
            na, det = rnd.pick((0, 1, 400, 4800, 5000)), rnd.pick((0, 1))
            if B >= 255 and g[2] > 40:
                g = rnd.pick(grids[:8])                   # (tensors no launch could hold)
            up = 2 if mode in (CT_FWD, CT_DGRAD) else st
            fine, coarse = g, tuple(max(v // up, 1) for v in g)
            if mode == CT_FWD:
                fine, coarse = tuple(2 * v for v in g), g
            si, so = (fine, coarse) if mode in (FWD, CT_DGRAD) else (coarse, fine)
            sparse = obs is not None
            o = obs or 0
            ibs = o + (1 if st == 2 and mode == FWD else 0) - (1 if st == 2 and mode == DGRAD and o > 0 else 0)
            rows.append((mode, dt, k, st, B, *si, cin, *so, cout, int(sparse), ibs if sparse else 0, o, na, acc, ep, part, det))
    return rows


def problems() -> np.ndarray:
    P = np.asarray(model_problems() + product_problems(), dtype=np.int32)
    assert P.shape[1] == len(COLS)
    return P


def digest(P: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(P, dtype=np.int32).tobytes()).hexdigest()


def cu_count() -> int:
    """what am_cu_count answers: the visible device's compute units, 256 without a device"""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def ask(P: np.ndarray) -> dict:
    sys.path.insert(0, ROOT)
    from anatomask_amd import hip
    L = hip.HipLib()._lib
    n = len(P)
    ans = {a: np.zeros(n, dtype=np.int64) for a in ANSWERS}
    rows, nbytes = C.c_int(0), C.c_long(0)
    for i, r in enumerate(P.tolist()):
        mode, dt, k, st, B, Di, Hi, Wi, Cin, Do, Ho, Wo, Cout, sparse, ibs, obs, na, acc, ep, part, det = r
        ans["uses_k3"][i] = L.am_conv3d_uses_k3(mode, dt, k, st, B, Di, Hi, Wi, Cin, Do, Ho, Wo, Cout, sparse, acc, ep, part)
        assert L.am_conv3d_partials_rows(mode, dt, k, st, B, Do, Ho, Wo, Cin, Cout, sparse, obs, na, C.byref(rows)) == 0
        ans["partials_rows"][i] = rows.value
        ans["prenorm_supported"][i] = L.am_conv3d_prenorm_supported(mode, dt, k, st, B, Do, Ho, Wo, Cin, Cout, sparse, ibs, obs, na)
        ans["wgrad_uses_k3"][i] = L.am_conv3d_wgrad_uses_k3(mode, dt, k, st, B, Do, Ho, Wo, Cin, Cout, sparse, det)
        fd, fh, fw = (max(v >> obs, 1) for v in (Do, Ho, Wo))
        assert L.am_conv3d_wgrad_gather_bytes(mode, dt, k, st, B, Cin, Cout, obs, sparse, na, fd, fh, fw, C.byref(nbytes)) == 0
        ans["wgrad_gather_bytes"][i] = nbytes.value
    return ans


if __name__ == "__main__":
    P = problems()
    ans = ask(P)
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    np.savez_compressed(OUT, problems_sha256=np.array(digest(P)), commit=np.array(commit), cu_count=np.array(cu_count()), **ans)
    print(OUT, len(P), "problems", os.path.getsize(OUT), "bytes", {a: int((v != 0).sum()) for a, v in ans.items()})
