"""The trainable STUNet segmentation network on the HIP engine: segmentation.STUNet with a backward.

    net = seg_train.STUNet(1, K, depth, dims).to(dev)                     # same constructor, same state_dict keys as segmentation.STUNet
    net.load_state_dict(checkpoint.encoder_weights_for_finetuning(...), strict=False)
    loss = seg_loss.build_loss(5, True)(net(data), targets)               # five fp32 logits tensors, finest first (or one)
    loss.backward()                                                       # .grad of every parameter
    torch.optim.SGD(net.parameters(), ...).step()

segmentation.STUNet stays inference-only (it refuses to run with gradients enabled); this subclass differs from it in `forward` alone: with
gradients enabled the network is ONE torch.autograd.Function around the engine's hand-written tape (engine.seg_forward(tape=...) /
engine.seg_backward), as modules._EncoderFn is around the pretraining encoder.  Its backward takes the logit gradients, runs
ops.seg_head_bwd per level and engine.seg_backward per sample, and returns the parameter gradients, which torch accumulates into .grad.
The gradient with respect to the input volume is not provided (None).  Under torch.no_grad(), or when no parameter requires a gradient,
the forward is exactly the parent's inference path.  No trainer, no DDP and no fused optimizer here: any torch optimizer steps the
fp32 master parameters, and the next forward repacks their compute-dtype copies."""
from __future__ import annotations

import torch

from . import engine, ops, segmentation

__all__ = ["STUNet"]


class _SegFn(torch.autograd.Function):
    """logits = STUNet(x): forward keeps one tape per sample (all B of them until backward: a batch loss couples the samples)."""

    @staticmethod
    def forward(ctx, net: "STUNet", inp, *params):
        W, pk = net._engine_ctx()
        ds = bool(net.decoder.deep_supervision)
        tape: list = []
        levels = engine.seg_forward(W, pk, inp, net.depth, all_levels=ds, tape=tape)
        feats = list(levels) if ds else [None] * 4 + [levels[0]]          # level u -> features (coarse -> fine)
        segs = [None if f is None else ops.seg_head(f, *net._head(u)) for u, f in enumerate(feats)]
        ctx.net, ctx.tape, ctx.inp, ctx.feats = net, tape, inp, feats
        ctx.set_materialize_grads(False)                                   # an unused output arrives as None, not as a tensor of zeros
        if not ds:
            return segs[4]
        return tuple([segs[4]] + segs[:4][::-1])                           # finest first (the reference's order)

    @staticmethod
    def backward(ctx, *dlogits):
        net, tape, inp, feats = ctx.net, ctx.tape, ctx.inp, ctx.feats
        if tape is None:
            raise RuntimeError("a second backward through the same STUNet forward: run the forward again")
        W, pk = net._engine_ctx()
        names = [engine.NET + "." + n for n, _ in net.named_parameters()]
        G = {n: torch.zeros_like(p.data, dtype=torch.float32) for n, (_, p) in zip(names, net.named_parameters())}
        by_level = [None] * 5                                              # output i -> level: 0 -> 4, then 3, 2, 1, 0
        for i, g in enumerate(dlogits):
            by_level[4 if i == 0 else 4 - i] = g
        dfeat = [None] * 5
        for u, g in enumerate(by_level):
            if g is None or feats[u] is None:
                continue
            hw, _ = net._head(u)
            dfeat[u] = ops.seg_head_bwd(g.float().contiguous(), feats[u], hw, G[f"{engine.NET}.seg_outputs.{u}.weight"],
                                        G[f"{engine.NET}.seg_outputs.{u}.bias"])
        for bi in range(inp.shape[0]):
            engine.seg_backward(W, G, pk, inp[bi:bi + 1], net.depth, tape[bi], [None if d is None else d[bi:bi + 1] for d in dfeat])
            tape[bi] = None                                                # free the sample's activations as we go
        ctx.tape = ctx.feats = None
        used = [feats[u] is not None for u in range(5)]
        grads = []
        for n in names:
            head = n.startswith(f"{engine.NET}.seg_outputs.")
            grads.append(G[n] if not head or used[int(n.split(".")[-2])] else None)
        return (None, None, *grads)


class STUNet(segmentation.STUNet):
    """segmentation.STUNet (P/STUNet.py:10-93) with gradients with respect to its parameters.  Same constructor, state_dict keys and
    `compute_dtype` switch; a state dict of either class loads into the other."""

    def forward(self, x):
        """x (B,1,D,H,W) fp32 -> logits (B,K,D,H,W) fp32, or with deep supervision the tuple of the five levels' logits, finest first.
        Differentiable with respect to the parameters when gradients are enabled and a parameter requires one."""
        params = [p for _, p in self.named_parameters()]
        if not torch.is_grad_enabled() or not any(p.requires_grad for p in params):
            return super().forward(x)
        self._check_input(x)
        return _SegFn.apply(self, x[:, 0].float().contiguous(), *params)
