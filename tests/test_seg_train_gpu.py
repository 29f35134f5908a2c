"""GPU: the gradients of the segmentation STUNet (anatomask_amd.seg_train, engine.seg_backward, seg_bwd_ops.hip) against fp64 torch
autograd on the CPU: einsum / repeat_interleave for the two kernels, tests/seg_oracle.forward + tests/seg_loss_oracle for the network.

Kernel bounds: dw, db, fp32 df / du relative L2 <= 1e-6 (fp32 arithmetic throughout: test_head_plain's bound for the forward head); bf16
df / du <= 2^-8 relative PER ELEMENT against the fp64 value (bf16 keeps 8 significant bits: one round-to-nearest store costs up to
2^-8 / (1 + 2^-8) = 3.891e-3 just above a power of two, which leaves 1.5e-5 for the fp32 sum; measured 3.89e-3).  A per-element
relative bound only means something for a sum that does not cancel (an fp32 sum of mixed signs has no relative accuracy near zero), so the
bf16 cases draw the summed operands (dlogits, w, the pre-filled df; dy) positive.  db at K = 1 is a single number under a relative L2
bound, so dlogits is positive in every case; the features (dw) are signed everywhere and w, the pre-filled df and dy in the fp32 cases.

Network, fp32 storage: every parameter's .grad against the fp64 oracle, per-tensor relative L2 <= 4 x e32, e32 = the worst per-tensor
error of the SAME oracle run in torch fp32 on the CPU, measured in the test (4 = the project's 3 x headroom plus one for the different
reduction trees: atomics in conv3d_wgrad, MFMA lane order).  conv1.bias / conv2.bias sit in front of an InstanceNorm (true gradient 0):
|g|_inf over the norm of the sibling norm*.bias gradient <= 16 x the worst such ratio of the CPU-fp32 run.  seg_outputs.0.* (weight 0 in
the loss) exactly zero; everything else non-zero in fp64 (106 of 130 tensors at depth [1] * 6).
Network, bf16 storage: whole-vector relative L2 of the encoder / decoder / head groups <= 2 x the same group's error of torch's CPU bf16
autocast of the oracle (the rounding points differ: the engine stores y1 / a1 / y2 / out in bf16, autocast rounds conv outputs only).
The autocast run uses torch's own CPU kernels (oneDNN switched off for it): oneDNN's bf16 convolutions are chosen by the host CPU's
instruction set, and with identical inputs its gradients were 0.304 / 0.195 / 0.0042 (encoder / decoder / heads) off the fp64 ones on
a host with AMX and 0.577 / 0.530 / 0.0040 on another, so the bound moved by a factor of two with the machine; torch's kernels gave
0.308 / 0.197 / 0.0041 where both were measured.  The engine's side does not move: a second forward + backward gives bit-equal logits
and gradients equal to 1e-4 per tensor, also on memory pre-filled with NaN patterns (test_backward_reads_no_uninitialised_memory_and_repeats).
End to end: 20 SGD steps on one batch lower the loss by more than half of what the fp64 oracle's own 20 steps achieve.

Measured on MI355X (printed by the tests): see DESIGN.md 5."""
import functools

import pytest
import torch

from anatomask_amd import ops, seg_loss, seg_train, segmentation as S
from anatomask_amd.data import deep_supervision_targets
from tests import seg_loss_oracle as LO
from tests import seg_oracle as SO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY_BF16 = 4e-2                                   # tests/test_segmentation_gpu.py's bound of the bf16 forward
SCALES = [1, 1 / 2, 1 / 4, 1 / 8, 1 / 16]
K_TINY = SO.TINY["num_classes"]


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm())


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("K", [1, 3, 105])
@pytest.mark.parametrize("C,shape", [(32, (2, 16, 8, 24)), (8, (2, 5, 6, 7)), (512, (1, 2, 4, 2)),
                                     (64, (2, 4, 6, 8)),        # at K = 105: features staged in LDS, weights read from global memory
                                     (128, (1, 3, 5, 8))])      # at K = 105: 65 984 bytes of LDS, the opt-in above 64 KB
def test_seg_head_bwd(C, shape, K, dtype, accumulate):
    g = torch.Generator().manual_seed(1000 * C + 10 * K + accumulate)
    # (see the module docstring: a bound on single elements needs sums that do not cancel; db is ONE number at K = 1)
    positive = lambda *s: torch.rand(*s, generator=g) + 0.5      # noqa: E731
    draw = positive if dtype == torch.bfloat16 else (lambda *s: torch.randn(*s, generator=g))
    B = shape[0]
    f = torch.randn(*shape, C, generator=g).to(dtype)
    dl = positive(B, K, *shape[1:])
    w = draw(K, C) / C ** 0.5
    df0 = draw(*shape, C).to(dtype)
    dw0, db0 = torch.randn(K, C, generator=g), torch.randn(K, generator=g)
    # fp64 autograd of the forward head
    fr, wr, br = f.double().requires_grad_(True), w.double().requires_grad_(True), torch.zeros(K, dtype=torch.float64, requires_grad=True)
    logits = torch.einsum("bdhwc,kc->bkdhw", fr, wr) + br[None, :, None, None, None]
    logits.backward(dl.double())
    want_df = fr.grad + (df0.double() if accumulate else 0)
    want_dw, want_db = dw0.double() + wr.grad, db0.double() + br.grad

    def run():
        dw, db = dw0.to(DEV), db0.to(DEV)
        df = ops.seg_head_bwd(dl.to(DEV), f.to(DEV), w.to(DEV), dw, db, df=df0.to(DEV).clone(), accumulate=accumulate)
        return df, dw, db
    df, dw, db = run()
    e_dw, e_db = _rel(dw, want_dw), _rel(db, want_db)
    assert df.dtype == dtype and e_dw <= 1e-6 and e_db <= 1e-6, (e_dw, e_db)
    if dtype == torch.float32:
        e_df = _rel(df, want_df)
        assert e_df <= 1e-6, e_df
    else:
        e_df = float(((df.double().cpu() - want_df).abs() / want_df.abs()).max())
        assert e_df <= 2.0 ** -8, e_df
    print(f"seg_head_bwd C={C} K={K} {dtype} accumulate={accumulate}: dw {e_dw:.2e} db {e_db:.2e} df {e_df:.2e}")
    again = run()
    assert all(torch.equal(a, b) for a, b in zip((df, dw, db), again))
    if dtype == torch.bfloat16:
        # mixed signs: the fp32 fma chain of K products (+ the stored df) is within (K + 1) 2^-24 S of the exact sum, S = the sum of the
        # terms' magnitudes; the bf16 store adds 2^-8 / (1 + 2^-8) of the computed value: |error| <= 2^-8 |exact| + (K + 2) 2^-24 S (K <= 255)
        sdl, sw = torch.randn(B, K, *shape[1:], generator=g), torch.randn(K, C, generator=g) / C ** 0.5
        sdf0 = torch.randn(*shape, C, generator=g).to(dtype)
        exact = torch.einsum("bkdhw,kc->bdhwc", sdl.double(), sw.double()) + (sdf0.double() if accumulate else 0)
        S = torch.einsum("bkdhw,kc->bdhwc", sdl.double().abs(), sw.double().abs()) + (sdf0.double().abs() if accumulate else 0)
        got = ops.seg_head_bwd(sdl.to(DEV), f.to(DEV), sw.to(DEV), dw0.to(DEV), db0.to(DEV), df=sdf0.to(DEV).clone(), accumulate=accumulate)
        excess = ((got.double().cpu() - exact).abs() - 2.0 ** -8 * exact.abs()) / S
        assert float(excess.max()) <= (K + 2) * 2.0 ** -24, float(excess.max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_seg_head_bwd_more_than_256_classes(dtype):
    """K = 300 runs as two launches of 256 and 44 classes: dw / db per chunk, df accumulated over the chunks.  fp32: the bounds above.
    bf16: df is rounded once per chunk, so two stores of at most u = 2^-8 / (1 + 2^-8) each (positive terms: the first chunk's part is
    no larger than the whole) plus the fp32 chains: <= 2 u + u^2 + K 2^-23 < 2^-7 + K 2^-23 per element."""
    K, C, shape = 300, 16, (1, 4, 5, 6)
    g = torch.Generator().manual_seed(300)
    f = torch.randn(*shape, C, generator=g).to(dtype)
    dl, w = torch.rand(1, K, *shape[1:], generator=g) + 0.5, (torch.rand(K, C, generator=g) + 0.5) / C ** 0.5
    dw0, db0 = torch.randn(K, C, generator=g), torch.randn(K, generator=g)
    dw, db = dw0.to(DEV), db0.to(DEV)
    df = ops.seg_head_bwd(dl.to(DEV), f.to(DEV), w.to(DEV), dw, db)
    want_df = torch.einsum("bkdhw,kc->bdhwc", dl.double(), w.double())
    want_dw = dw0.double() + torch.einsum("bkdhw,bdhwc->kc", dl.double(), f.double())
    want_db = db0.double() + dl.double().sum((0, 2, 3, 4))
    assert _rel(dw, want_dw) <= 1e-6 and _rel(db, want_db) <= 1e-6
    if dtype == torch.float32:
        assert _rel(df, want_df) <= 1e-6
    else:
        e = float(((df.double().cpu() - want_df).abs() / want_df.abs()).max())
        print(f"seg_head_bwd K=300 bf16: df {e:.3e}")
        assert e <= 2.0 ** -7 + K * 2.0 ** -23, e


def test_seg_head_bwd_allocates_df_and_checks_its_workspace():
    f = torch.randn(1, 4, 4, 4, 8, device=DEV)
    dl, w = torch.randn(1, 2, 4, 4, 4, device=DEV), torch.randn(2, 8, device=DEV)
    dw, db = torch.zeros(2, 8, device=DEV), torch.zeros(2, device=DEV)
    df = ops.seg_head_bwd(dl, f, w, dw, db)
    assert _rel(df, torch.einsum("bkdhw,kc->bdhwc", dl.double(), w.double())) <= 1e-6
    from anatomask_amd import hip
    ws = torch.empty(4, device=DEV)
    with pytest.raises(RuntimeError, match="am_seg_head_bwd"):          # a workspace smaller than the header's formula launches nothing
        hip.lib().seg_head_bwd(hip.DT_F32, dl.data_ptr(), f.data_ptr(), w.data_ptr(), 1, 4, 4, 4, 8, 2, df.data_ptr(), 0, dw.data_ptr(),
                               db.data_ptr(), ws.data_ptr(), ws.numel(), None)
    with pytest.raises(RuntimeError, match="am_seg_head_bwd"):          # C % 8
        ops.seg_head_bwd(torch.randn(1, 2, 4, 4, 4, device=DEV), torch.randn(1, 4, 4, 4, 12, device=DEV), torch.randn(2, 12, device=DEV),
                         torch.zeros(2, 12, device=DEV), db)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("factor", [1, 2])
def test_seg_upcat_bwd(dtype, factor):
    B, D, H, W, C = 2, 8, 16, 12, 24
    g = torch.Generator().manual_seed(7 + factor)
    dy = (torch.rand(B, D, H, W, 2 * C, generator=g) + 0.5 if dtype == torch.bfloat16 else torch.randn(B, D, H, W, 2 * C, generator=g)).to(dtype)
    u = torch.zeros(B, D // factor, H // factor, W // factor, C, dtype=torch.float64, requires_grad=True)
    skip = torch.zeros(B, D, H, W, C, dtype=torch.float64, requires_grad=True)
    up = u.repeat_interleave(factor, 1).repeat_interleave(factor, 2).repeat_interleave(factor, 3)
    torch.cat((up, skip), -1).backward(dy.double())
    du, dskip = ops.seg_upcat_bwd(dy.to(DEV), factor)
    assert du.dtype == dtype and tuple(du.shape) == tuple(u.shape)
    assert torch.equal(dskip.cpu(), dy[..., C:]) and torch.equal(dskip.double().cpu(), skip.grad)
    if dtype == torch.float32:
        e = _rel(du, u.grad)
        assert e <= 1e-6, e
    else:
        e = float(((du.double().cpu() - u.grad).abs() / u.grad.abs()).max())
        assert e <= 2.0 ** -8, e
    print(f"seg_upcat_bwd factor {factor} {dtype}: du {e:.2e}")


def test_seg_upcat_bwd_bad_arguments_raise():
    for shape, factor in (((1, 4, 4, 4, 24), 2),        # C = 12: not a multiple of 8
                          ((1, 6, 6, 6, 16), 3),        # factor 3
                          ((1, 4, 5, 4, 16), 2),        # an odd size with factor 2
                          ((1, 3, 4, 4, 16), 2)):
        with pytest.raises(RuntimeError, match="am_seg_upcat_bwd"):
            ops.seg_upcat_bwd(torch.zeros(*shape, device=DEV), factor)


# ------------------------------------------------------------------ network
def _keys(depth):
    return SO.state_keys(SO.TINY["dims"], depth, K_TINY)


@functools.lru_cache(maxsize=None)
def _case(size, depth):
    """(weights, x [2,1,*size], labels int16 [2,1,*size]): two different smooth samples, blob labels at the 0.6 / 0.85 quantiles."""
    W = SO.seeded_weights(_keys(list(depth)), 1234)
    x = torch.stack([SO.smooth_input(size, 77), SO.smooth_input(size, 78)])[:, None]
    blob = torch.stack([SO.smooth_input(size, 31), SO.smooth_input(size, 32)])[:, None]
    q = torch.quantile(blob.flatten(), torch.tensor([0.6, 0.85]))
    labels = ((blob > q[0]).to(torch.int16) + (blob > q[1]).to(torch.int16))
    return W, x, labels


def _oracle_loss(outs, labels):
    return LO.deep_supervision(lambda a, t: LO.dice_ce(a, t, True), outs, deep_supervision_targets(labels, SCALES), LO.nnunet_weights(5))


@functools.lru_cache(maxsize=None)
def _oracle(size, depth, mode):
    """(loss, logits, {name: gradient}) of the CPU oracle: mode 'f64', 'f32' or 'autocast' (torch's CPU bf16 autocast of the fp32 oracle)."""
    W, x, labels = _case(size, depth)
    dt = torch.float64 if mode == "f64" else torch.float32
    Wd = {k: v.detach().to(dt).requires_grad_(True) for k, v in W.items()}
    # (autocast: oneDNN off, forward and backward.  Its bf16 convolutions depend on the host CPU's instruction set -- the same inputs gave
    # whole-vector encoder errors of 0.30 on one host and 0.58 on another -- torch's own kernels do not; see the module docstring)
    with torch.backends.mkldnn.flags(enabled=mode != "autocast"):
        if mode == "autocast":
            with torch.autocast("cpu", dtype=torch.bfloat16):
                outs = SO.forward(Wd, x.to(dt), list(depth), deep_supervision=True)
            outs = [o.float() for o in outs]
        else:
            outs = SO.forward(Wd, x.to(dt), list(depth), deep_supervision=True)
        loss = _oracle_loss(outs, labels)
        grads = torch.autograd.grad(loss, list(Wd.values()), allow_unused=True)
    return loss.detach(), [o.detach() for o in outs], {k: (torch.zeros_like(w) if g is None else g.detach()) for (k, w), g in zip(Wd.items(), grads)}


def _net(W, depth, dtype, cls=seg_train.STUNet):
    net = cls(1, K_TINY, depth=list(depth), dims=SO.TINY["dims"], enable_deep_supervision=True)
    net.load_state_dict(W)
    net.compute_dtype = dtype
    return net.to(DEV)


def _engine(size, depth, dtype):
    """(net, loss, logits, {name: .grad}) of one forward + loss + backward on the engine."""
    W, x, labels = _case(size, depth)
    net = _net(W, depth, dtype)
    outs = net(x.to(DEV))
    loss = seg_loss.build_loss(5, True)(outs, deep_supervision_targets(labels.to(DEV), SCALES))
    loss.backward()
    return net, loss.detach(), [o.detach() for o in outs], {k: p.grad.detach().clone() for k, p in net.named_parameters()}


def _is_prenorm_bias(k):
    return k.endswith((".conv1.bias", ".conv2.bias"))


@pytest.mark.parametrize("size,depth", [((32, 32, 32), (1,) * 6), ((16, 32, 48), (1,) * 6), ((32, 32, 32), (1, 2, 1, 1, 1, 1))])
def test_network_gradients_fp32(size, depth):
    W, x, labels = _case(size, depth)
    l64, o64, g64 = _oracle(size, depth, "f64")
    _, _, g32 = _oracle(size, depth, "f32")
    net, loss, outs, g = _engine(size, depth, torch.float32)
    assert set(g) == set(g64) and len(outs) == 5
    assert abs(float(loss) - float(l64)) <= 1e-4 * abs(float(l64)), (float(loss), float(l64))
    # the tape does not change the forward: the inference network on the same weights gives the same bits
    ref = _net(W, depth, torch.float32, S.STUNet).requires_grad_(False)
    with torch.no_grad():
        plain = ref(x.to(DEV))
        same = net(x.to(DEV))
    for a, b, c in zip(outs, plain, same):
        assert torch.equal(a, b) and torch.equal(c, b)
    zero = [k for k in g64 if k.startswith("seg_outputs.0.")]
    bias = [k for k in g64 if _is_prenorm_bias(k)]
    live = [k for k in g64 if k not in zero and k not in bias]
    assert len(zero) == 2 and len(bias) == 2 * (sum(depth) + sum(depth[:5])) and all(float(g64[k].abs().max()) > 0 for k in live)
    if depth == (1,) * 6:
        assert len(g64) == 130 and len(live) == 106
    for k in zero:
        assert float(g64[k].abs().max()) == 0.0 and float(g[k].abs().max()) == 0.0, k
    e32 = max(_rel(g32[k], g64[k]) for k in live)
    errs = {k: _rel(g[k], g64[k]) for k in live}
    worst = max(errs, key=errs.get)
    whole = _rel(torch.cat([g[k].flatten().cpu() for k in live]), torch.cat([g64[k].flatten() for k in live]))
    print(f"seg_train fp32 {size} depth {depth}: e32 {e32:.3e}, engine worst {errs[worst]:.3e} ({worst}), whole vector {whole:.3e}")
    assert errs[worst] <= 4 * e32, (worst, errs[worst], e32)
    sib = lambda k: g64[k.replace(".conv", ".norm")].norm()      # noqa: E731  (conv1.bias -> norm1.bias)
    r32 = max(float(g32[k].abs().max() / sib(k)) for k in bias)
    rge = {k: float(g[k].abs().max().cpu() / sib(k)) for k in bias}
    wb = max(rge, key=rge.get)
    print(f"  pre-norm conv biases (true gradient 0): |g|inf / |norm bias grad|  CPU fp32 {r32:.3e}, engine worst {rge[wb]:.3e} ({wb})")
    assert rge[wb] <= 16 * r32, (wb, rge[wb], r32)
    # a second backward from a fresh forward ADDS to .grad
    loss2 = seg_loss.build_loss(5, True)(net(x.to(DEV)), deep_supervision_targets(labels.to(DEV), SCALES))
    loss2.backward()
    for k, p in net.named_parameters():
        if k in live:
            assert _rel(p.grad, 2 * g[k]) <= 1e-5, k


def test_one_output_and_unused_outputs():
    """enable_deep_supervision=False (one logits tensor, the heads of levels 0-3 unused: their .grad stays None) against the fp64 oracle
    under the same 4 x e32 rule; and the five-output network with a loss on its finest output alone (the other four arrive in backward
    as None) gives the same gradients."""
    size, depth = (32, 32, 32), (1,) * 6
    W, x, labels = _case(size, depth)
    grads = {}
    for dt in (torch.float64, torch.float32):
        Wd = {k: v.detach().to(dt).requires_grad_(True) for k, v in W.items()}
        loss = LO.dice_ce(SO.forward(Wd, x.to(dt), list(depth)), labels, True)
        grads[dt] = dict(zip(Wd, torch.autograd.grad(loss, list(Wd.values()), allow_unused=True)))
    g64, g32 = grads[torch.float64], grads[torch.float32]
    live = [k for k in g64 if g64[k] is not None and not _is_prenorm_bias(k)]
    assert sorted(k for k in g64 if g64[k] is None) == sorted(f"seg_outputs.{u}.{n}" for u in range(4) for n in ("weight", "bias"))
    e32 = max(_rel(g32[k], g64[k]) for k in live)
    loss_fn = seg_loss.DC_and_CE_loss({"batch_dice": True, "smooth": 1e-5, "do_bg": False, "ddp": False}, {}, weight_ce=1, weight_dice=1,
                                      ignore_label=None, dice_class=seg_loss.MemoryEfficientSoftDiceLoss)      # build_loss's level loss
    got = {}
    for ds in (False, True):
        net = seg_train.STUNet(1, K_TINY, depth=list(depth), dims=SO.TINY["dims"], enable_deep_supervision=ds)
        net.load_state_dict(W)
        net = net.to(DEV)
        out = net(x.to(DEV))
        assert isinstance(out, tuple) == ds
        loss_fn(out[0] if ds else out, labels.to(DEV)).backward()
        got[ds] = {k: p.grad for k, p in net.named_parameters()}
    errs = {k: _rel(got[False][k], g64[k]) for k in live}
    worst = max(errs, key=errs.get)
    print(f"seg_train one output fp32: e32 {e32:.3e}, engine worst {errs[worst]:.3e} ({worst})")
    assert errs[worst] <= 4 * e32, (worst, errs[worst], e32)
    for u in range(4):
        assert got[False][f"seg_outputs.{u}.weight"] is None and got[False][f"seg_outputs.{u}.bias"] is None
        assert float(got[True][f"seg_outputs.{u}.weight"].abs().max()) == 0.0
    for k in live:
        assert _rel(got[True][k], got[False][k]) <= 1e-5, k


def _poison_allocator():
    """fill blocks of many sizes with 0xFFFF (a NaN in bf16 and in fp32) and hand them back to torch's caching allocator: the next
    torch.empty of a similar size gets them."""
    keep = []
    for sh in range(9, 28):
        for _ in range(6 if sh < 24 else 2):
            keep.append(torch.full(((1 << sh) // 2,), -1, dtype=torch.int16, device=DEV))
    torch.cuda.synchronize()
    del keep


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_backward_reads_no_uninitialised_memory_and_repeats(dtype):
    """the forward is deterministic and of the backward only the convolution weight gradients add with fp32 atomics: a second run, made on
    allocator blocks that hold NaN patterns, gives bit-equal logits and the same gradients to 1e-4 per tensor (measured: 0 tensors differ)."""
    size, depth = (32, 32, 32), (1,) * 6
    _, _, o0, g0 = _engine(size, depth, dtype)
    _poison_allocator()
    _, _, o1, g1 = _engine(size, depth, dtype)
    assert all(torch.equal(a, b) for a, b in zip(o0, o1))
    for k in g0:
        assert bool(torch.isfinite(g1[k]).all()), k
        assert float((g0[k] - g1[k]).norm()) <= 1e-4 * float(g0[k].norm()), k


def _group(k):
    return "heads" if k.startswith("seg_outputs.") else "encoder" if k.startswith("conv_blocks_context.") else "decoder"


def test_network_gradients_bf16():
    size, depth = (32, 32, 32), (1,) * 6
    _, o64, g64 = _oracle(size, depth, "f64")
    _, _, gac = _oracle(size, depth, "autocast")
    _, _, outs, g = _engine(size, depth, torch.bfloat16)
    ef = max(_rel(a, b) for a, b in zip(outs, o64))
    print(f"seg_train bf16 {size}: logits vs fp64 oracle {ef:.3e}")
    assert ef <= TINY_BF16
    for grp in ("encoder", "decoder", "heads"):
        ks = [k for k in g64 if _group(k) == grp]
        cat = lambda d: torch.cat([d[k].flatten().double().cpu() for k in ks])      # noqa: E731
        e_eng, e_ac = _rel(cat(g), cat(g64)), _rel(cat(gac), cat(g64))
        print(f"  {grp}: whole-vector rel L2 engine {e_eng:.3e}, CPU bf16 autocast {e_ac:.3e}")
        assert e_eng <= 2 * e_ac, (grp, e_eng, e_ac)


@functools.lru_cache(maxsize=None)
def _oracle_descent(steps):
    size, depth = (32, 32, 32), (1,) * 6
    W, x, labels = _case(size, depth)
    P = [v.detach().double().requires_grad_(True) for v in W.values()]
    opt = torch.optim.SGD(P, lr=1e-2, momentum=0.9)
    losses = []
    for _ in range(steps + 1):
        opt.zero_grad()
        loss = _oracle_loss(SO.forward(dict(zip(W, P)), x.double(), list(depth), deep_supervision=True), labels)
        losses.append(float(loss.detach()))
        if len(losses) <= steps:
            loss.backward()
            opt.step()
    return losses[0], losses[-1]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_twenty_sgd_steps_descend(dtype):
    size, depth, steps = (32, 32, 32), (1,) * 6, 20
    W, x, labels = _case(size, depth)
    net = _net(W, depth, dtype)
    opt = torch.optim.SGD(net.parameters(), lr=1e-2, momentum=0.9)
    loss_fn = seg_loss.build_loss(5, True)
    xd, targets = x.to(DEV), deep_supervision_targets(labels.to(DEV), SCALES)
    losses = []
    for _ in range(steps + 1):
        opt.zero_grad()
        loss = loss_fn(net(xd), targets)
        losses.append(loss.detach())
        if len(losses) <= steps:
            loss.backward()
            opt.step()
    first, last = float(losses[0]), float(losses[-1])
    o_first, o_last = _oracle_descent(steps)
    print(f"seg_train {dtype}: loss {first:.5f} -> {last:.5f} after {steps} SGD steps; fp64 oracle {o_first:.5f} -> {o_last:.5f}")
    assert o_first - o_last > 0
    assert first - last > 0.5 * (o_first - o_last), (first, last, o_first, o_last)
