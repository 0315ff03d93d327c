"""Host-side mirror of the variational sample and the loss terms (scope row f-3):

    reference                                                                          here
    ---------------------------------------------------------------------------------  ------------------------------
    sample(μ, logσ²) = μ + ε·exp(logσ²/2)   [REF GOKU.jl:155-163], [REF LatentODE.jl:82-89]     sample(mu, logvar)
    sample + β·vector_kl of the same (μ, logσ²), as loss_batch uses them                         sample_with_kl(mu, logvar, β, B)
    kl(μ, logσ²), vector_kl                  [REF src/utils/utils.jl:15-49]                      kl, vector_kl
    reconstruction_loss = sum(mean((x − x̂)², dims=(2,3)))   [REF model_train.jl:225-238]        reconstruction_loss

On HIP tensors every function is one liblde.so kernel (two for the reductions) forward and one backward
(lde_sample_* / lde_kl_* / lde_mse_*, include/lde.h): no chain of broadcast kernels, no host synchronisation. ε is drawn
by lde_randn from the state of torch's CUDA generator (`randn` below), like the reference draws it with randn. There is no CPU path.

β, the KL weight, is a Python / numpy number — it then travels as a kernel argument, β/B formed on the host — or a β WORD: a float32 HIP
tensor of one element, read by the kernels at run time (the lde_*_dev entry points: s = β ⊘ B, one f32 division on the device). A captured
training step whose β is a word follows the schedule by the host writing into the word between replays (train.train(graphed=True)).
β gets no gradient. A β tensor on the CPU is read as the number it holds, once, at the call."""
from __future__ import annotations


import torch

from . import _lib as L


def _stream():
    return L.raw_stream()


def _need_gpu(t):
    L.need_gpu(t.is_cuda, "a loss kernel")


class _SampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, logvar, eps):
        _need_gpu(mu)
        mu, logvar = mu.contiguous().float(), logvar.contiguous().float()
        out = torch.empty_like(mu)
        L.call("lde_sample_forward", None, L.ptr(mu), L.ptr(logvar), L.ptr(eps), mu.numel(), L.ptr(out), _stream())
        ctx.save_for_backward(logvar, eps)
        return out

    @staticmethod
    def backward(ctx, dl):
        logvar, eps = ctx.saved_tensors
        dl = dl.contiguous()
        dlv = torch.empty_like(logvar)
        L.call("lde_sample_backward", None, L.ptr(logvar), L.ptr(eps), L.ptr(dl), dl.numel(), L.ptr(dlv), _stream())
        return dl, dlv, None


class _KlFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, logvar, scale):
        _need_gpu(mu)
        mu, logvar = mu.contiguous().float(), logvar.contiguous().float()
        ws, p_out, p_scratch = L.loss_scratch(mu.device)
        L.call("lde_kl_forward", None, L.ptr(mu), L.ptr(logvar), mu.numel(), scale, p_out, p_scratch, _stream())
        ctx.save_for_backward(mu, logvar)
        ctx.scale = scale
        return ws[0]

    @staticmethod
    def backward(ctx, g):
        mu, logvar = ctx.saved_tensors
        g = g.contiguous().float()
        dmu, dlv = torch.empty_like(mu), torch.empty_like(logvar)
        L.call("lde_kl_backward", None, L.ptr(mu), L.ptr(logvar), mu.numel(), ctx.scale, L.ptr(g), L.ptr(dmu), L.ptr(dlv), _stream())
        return dmu, dlv, None


class _MseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, xhat, scale):
        _need_gpu(xhat)
        ws, p_out, p_scratch = L.loss_scratch(xhat.device)
        L.call("lde_mse_forward", None, L.ptr(x), L.ptr(xhat), xhat.numel(), scale, p_out, p_scratch, _stream())
        ctx.save_for_backward(x, xhat)
        ctx.scale = scale
        return ws[0]

    @staticmethod
    def backward(ctx, g):
        x, xhat = ctx.saved_tensors
        g = g.contiguous().float()
        dxh = torch.empty_like(xhat)
        L.call("lde_mse_backward", None, L.ptr(x), L.ptr(xhat), xhat.numel(), ctx.scale, L.ptr(g), L.ptr(dxh), _stream())
        return None, dxh, None


class _SampleKlFn(torch.autograd.Function):
    """(l̃, total) = (μ + ε·exp(logσ²/2), base + scale·Σ kl(μ, logσ²)): lde_sample_kl_forward / _backward — one pass each way
    over (μ, logσ²) for the sample AND its KL term; the pullback writes the summed cotangents."""

    @staticmethod
    def forward(ctx, mu, logvar, eps, scale, base):
        _need_gpu(mu)
        out = torch.empty_like(mu)
        ws, p_out, p_scratch = L.loss_scratch(mu.device)
        L.call("lde_sample_kl_forward", None, L.ptr(mu), L.ptr(logvar), L.ptr(eps), mu.numel(), scale, L.ptr(base), L.ptr(out), p_out, p_scratch,
               _stream())
        ctx.save_for_backward(mu, logvar, eps)
        ctx.scale, ctx.has_base = scale, base is not None
        return out, ws[0]

    @staticmethod
    def backward(ctx, dl, g):
        mu, logvar, eps = ctx.saved_tensors
        dl, g = dl.contiguous(), g.contiguous().float()
        dmu, dlv = torch.empty_like(mu), torch.empty_like(logvar)
        L.call("lde_sample_kl_backward", None, L.ptr(mu), L.ptr(logvar), L.ptr(eps), L.ptr(dl), L.ptr(g), ctx.scale, mu.numel(), L.ptr(dmu),
               L.ptr(dlv), _stream())
        return dmu, dlv, None, None, (g if ctx.has_base else None)


def beta_word(beta):
    """(word, number) of a β argument: a float32 HIP tensor of one element is a β word (detached: β gets no gradient); anything else —
    a Python or numpy number, a CPU tensor — is the number it holds."""
    if torch.is_tensor(beta):
        if beta.is_cuda:
            if beta.dtype != torch.float32 or beta.numel() != 1:
                raise TypeError("a β word is ONE float32 on the GPU")
            return beta.detach(), None
        return None, float(beta)
    return None, beta


def _same_device(word, t):
    if word.device != t.device:
        raise ValueError(f"the β word lives on {word.device}, the loss term on {t.device}")


class _KlDevFn(torch.autograd.Function):
    """base + (β ⊘ divisor)·Σ kl(μ, logσ²) with β a device word: lde_kl_forward_dev / lde_kl_backward_dev."""

    @staticmethod
    def forward(ctx, mu, logvar, word, divisor, base):
        _need_gpu(mu)
        _same_device(word, mu)
        mu, logvar = mu.contiguous().float(), logvar.contiguous().float()
        ws, p_out, p_scratch = L.loss_scratch(mu.device)
        L.call("lde_kl_forward_dev", None, L.ptr(mu), L.ptr(logvar), mu.numel(), L.ptr(word), divisor, L.ptr(base), p_out, p_scratch, _stream())
        ctx.save_for_backward(mu, logvar, word)
        ctx.divisor, ctx.has_base = divisor, base is not None
        return ws[0]

    @staticmethod
    def backward(ctx, g):
        mu, logvar, word = ctx.saved_tensors
        g = g.contiguous().float()
        dmu, dlv = torch.empty_like(mu), torch.empty_like(logvar)
        L.call("lde_kl_backward_dev", None, L.ptr(mu), L.ptr(logvar), mu.numel(), L.ptr(word), ctx.divisor, L.ptr(g), L.ptr(dmu), L.ptr(dlv), _stream())
        return dmu, dlv, None, None, (g if ctx.has_base else None)


class _SampleKlDevFn(torch.autograd.Function):
    """_SampleKlFn with β a device word: lde_sample_kl_forward_dev / _backward_dev (scale = β ⊘ divisor, formed by the kernel)."""

    @staticmethod
    def forward(ctx, mu, logvar, eps, word, divisor, base):
        _need_gpu(mu)
        _same_device(word, mu)
        out = torch.empty_like(mu)
        ws, p_out, p_scratch = L.loss_scratch(mu.device)
        L.call("lde_sample_kl_forward_dev", None, L.ptr(mu), L.ptr(logvar), L.ptr(eps), mu.numel(), L.ptr(word), divisor, L.ptr(base), L.ptr(out),
               p_out, p_scratch, _stream())
        ctx.save_for_backward(mu, logvar, eps, word)
        ctx.divisor, ctx.has_base = divisor, base is not None
        return out, ws[0]

    @staticmethod
    def backward(ctx, dl, g):
        mu, logvar, eps, word = ctx.saved_tensors
        dl, g = dl.contiguous(), g.contiguous().float()
        dmu, dlv = torch.empty_like(mu), torch.empty_like(logvar)
        L.call("lde_sample_kl_backward_dev", None, L.ptr(mu), L.ptr(logvar), L.ptr(eps), L.ptr(dl), L.ptr(g), L.ptr(word), ctx.divisor, mu.numel(),
               L.ptr(dmu), L.ptr(dlv), _stream())
        return dmu, dlv, None, None, None, (g if ctx.has_base else None)


class _MseAddFn(torch.autograd.Function):
    """base + scale·Σ (x − x̂)²: lde_mse_forward_add; the pullback is lde_mse_backward and passes the cotangent on to `base`."""

    @staticmethod
    def forward(ctx, x, xhat, scale, base):
        _need_gpu(xhat)
        ws, p_out, p_scratch = L.loss_scratch(xhat.device)
        L.call("lde_mse_forward_add", None, L.ptr(x), L.ptr(xhat), xhat.numel(), scale, L.ptr(base), p_out, p_scratch, _stream())
        ctx.save_for_backward(x, xhat)
        ctx.scale = scale
        return ws[0]

    @staticmethod
    def backward(ctx, g):
        x, xhat = ctx.saved_tensors
        g = g.contiguous().float()
        dxh = torch.empty_like(xhat)
        L.call("lde_mse_backward", None, L.ptr(x), L.ptr(xhat), xhat.numel(), ctx.scale, L.ptr(g), L.ptr(dxh), _stream())
        return None, dxh, None, g


def _same_layout(a: torch.Tensor, b: torch.Tensor):
    """a and b brought to contiguous buffers with the SAME element order; also returns the permutation applied to both
    (None when they were contiguous already) so that a caller can undo it — never inferred from shapes: a [16, 16] view
    permutes without changing its shape."""
    if a.shape != b.shape:
        raise ValueError("operands differ in shape")
    if a.is_contiguous() and b.is_contiguous():
        return a, b, None
    order = sorted(range(b.dim()), key=lambda d: -b.stride(d))
    a2, b2 = a.permute(order), b.permute(order)
    if not b2.is_contiguous():
        b2 = b2.contiguous()
    if not a2.is_contiguous():
        a2 = a2.contiguous()
    return a2, b2, (None if order == list(range(b.dim())) else order)


# ---- ε --------------------------------------------------------------------------------------------------------------------------
# lde_randn (Philox4x32-10 + Box–Muller, include/lde.h) driven by torch's CUDA generator: outside a capture every draw takes the
# generator's (seed, offset) and advances the offset like a torch draw of the same size would — torch.manual_seed reproduces a run, other
# torch draws interleave consistently — without launching anything but the one kernel. Inside a stream capture the host state is frozen
# into the graph, so the draw is keyed by the state last seen outside, a per-draw call index, and a DEVICE counter read by the kernel:
# the step count of the optimiser in the captured step (train.FluxADAMW(capturable=True) registers it) — fresh noise at every replay,
# none of the three fill / copy launches torch's graph-safe generator puts in front of a replay. No counter registered: torch.randn.
_NATIVE_RNG = True
_noise_epoch = {}          # device index → int64 device scalar that changes from replay to replay
_noise_base = {}           # device index → (seed, offset) of torch's generator when last seen outside a capture
_noise_call = [0]


def set_noise_epoch(counter):
    """Register (or with None, clear) the device int64 scalar that separates the replays of a captured step for `randn`."""
    if counter is None:
        _noise_epoch.clear()
        return
    if not (torch.is_tensor(counter) and counter.is_cuda and counter.dtype == torch.int64 and counter.numel() == 1):
        raise TypeError("set_noise_epoch: an int64 scalar on the GPU")
    _noise_epoch[counter.device.index] = counter


def _draw_key(n: int, idx: int):
    """(seed, offset, call, epoch pointer) of the next draw of n numbers on device idx, or None when torch.randn has to make it (the
    switch is off, or a capture without a registered counter). Advances the generator state like the draw."""
    capturing = torch.cuda.is_current_stream_capturing()
    if not _NATIVE_RNG or (capturing and (idx not in _noise_epoch or idx not in _noise_base)):
        return None
    if capturing:
        seed, off = _noise_base[idx]
        _noise_call[0] += 1
        return seed, (off + (1 << 40)) & 0xFFFFFFFFFFFFFFFF, _noise_call[0], L.ptr(_noise_epoch[idx])
    gen = torch.cuda.default_generators[idx]
    seed, off = gen.initial_seed() & 0xFFFFFFFFFFFFFFFF, gen.get_offset()
    gen.set_offset(off + 4 * ((n + 3) // 4))
    _noise_base[idx] = (seed, off + 4 * ((n + 3) // 4))
    return seed, off, 0, None


def randn(shape, device) -> torch.Tensor:
    """ε ~ N(0, 1) of the given shape on `device` (float32)."""
    device = torch.device(device)
    L.need_gpu(device.type == "cuda", "a loss kernel")
    idx = device.index if device.index is not None else torch.cuda.current_device()
    out = torch.empty(shape, device=device, dtype=torch.float32)
    key = _draw_key(out.numel(), idx)
    if key is None:
        return torch.randn(shape, device=device, dtype=torch.float32)
    seed, off, call, ep = key
    L.call("lde_randn", None, L.ptr(out), out.numel(), seed, off, call, ep, None, L.raw_stream(idx))
    return out


class _SampleKlPairFn(torch.autograd.Function):
    """((l̃_a, l̃_b), total) for the two parts of the GOKU tuple in ONE launch each way (lde_sample_kl_pair_forward / _backward): ε of both
    parts drawn inside the kernel with the keys `randn` would have used, the samples, and base + scale_a·Σ kl_a + scale_b·Σ kl_b. The same
    device code in the same order as randn → _SampleKlFn → randn → _SampleKlFn: the same bits
    (tests/test_gpu_loss.py::test_sample_pair_equals_the_separate_calls)."""

    @staticmethod
    def forward(ctx, mu_a, lv_a, mu_b, lv_b, scale_a, scale_b, keys):
        (seed, off_a, call_a, ep), (_, off_b, call_b, _) = keys
        eps_a, eps_b, l_a, l_b = torch.empty_like(mu_a), torch.empty_like(mu_b), torch.empty_like(mu_a), torch.empty_like(mu_b)
        ws, p_out, p_parts = L.loss_scratch(mu_a.device, 2)          # [0]: the total, then two partial sums
        L.call("lde_sample_kl_pair_forward", None, L.ptr(mu_a), L.ptr(lv_a), mu_a.numel(), scale_a, L.ptr(mu_b), L.ptr(lv_b), mu_b.numel(), scale_b,
               None, seed, off_a, off_b, call_a, call_b, ep, L.ptr(eps_a), L.ptr(eps_b), L.ptr(l_a), L.ptr(l_b), p_out, p_parts, _stream())
        ctx.save_for_backward(mu_a, lv_a, eps_a, mu_b, lv_b, eps_b)
        ctx.scales = (scale_a, scale_b)
        return l_a, l_b, ws[0]

    @staticmethod
    def backward(ctx, dl_a, dl_b, g):
        mu_a, lv_a, eps_a, mu_b, lv_b, eps_b = ctx.saved_tensors
        dl_a, dl_b, g = dl_a.contiguous(), dl_b.contiguous(), g.contiguous().float()
        dmu_a, dlv_a, dmu_b, dlv_b = torch.empty_like(mu_a), torch.empty_like(lv_a), torch.empty_like(mu_b), torch.empty_like(lv_b)
        L.call("lde_sample_kl_pair_backward", None, L.ptr(mu_a), L.ptr(lv_a), L.ptr(eps_a), L.ptr(dl_a), mu_a.numel(), ctx.scales[0], L.ptr(mu_b),
               L.ptr(lv_b), L.ptr(eps_b), L.ptr(dl_b), mu_b.numel(), ctx.scales[1], L.ptr(g), L.ptr(dmu_a), L.ptr(dlv_a), L.ptr(dmu_b), L.ptr(dlv_b),
               _stream())
        return dmu_a, dlv_a, dmu_b, dlv_b, None, None, None


class _SampleKlPairDevFn(torch.autograd.Function):
    """_SampleKlPairFn with β a device word: lde_sample_kl_pair_forward_dev / _backward_dev, one divisor per part."""

    @staticmethod
    def forward(ctx, mu_a, lv_a, mu_b, lv_b, word, div_a, div_b, keys):
        _same_device(word, mu_a)
        (seed, off_a, call_a, ep), (_, off_b, call_b, _) = keys
        eps_a, eps_b, l_a, l_b = torch.empty_like(mu_a), torch.empty_like(mu_b), torch.empty_like(mu_a), torch.empty_like(mu_b)
        ws, p_out, p_parts = L.loss_scratch(mu_a.device, 2)          # [0]: the total, then two partial sums
        L.call("lde_sample_kl_pair_forward_dev", None, L.ptr(mu_a), L.ptr(lv_a), mu_a.numel(), div_a, L.ptr(mu_b), L.ptr(lv_b), mu_b.numel(), div_b,
               L.ptr(word), None, seed, off_a, off_b, call_a, call_b, ep, L.ptr(eps_a), L.ptr(eps_b), L.ptr(l_a), L.ptr(l_b), p_out, p_parts, _stream())
        ctx.save_for_backward(mu_a, lv_a, eps_a, mu_b, lv_b, eps_b, word)
        ctx.divisors = (div_a, div_b)
        return l_a, l_b, ws[0]

    @staticmethod
    def backward(ctx, dl_a, dl_b, g):
        mu_a, lv_a, eps_a, mu_b, lv_b, eps_b, word = ctx.saved_tensors
        dl_a, dl_b, g = dl_a.contiguous(), dl_b.contiguous(), g.contiguous().float()
        dmu_a, dlv_a, dmu_b, dlv_b = torch.empty_like(mu_a), torch.empty_like(lv_a), torch.empty_like(mu_b), torch.empty_like(lv_b)
        L.call("lde_sample_kl_pair_backward_dev", None, L.ptr(mu_a), L.ptr(lv_a), L.ptr(eps_a), L.ptr(dl_a), mu_a.numel(), ctx.divisors[0],
               L.ptr(mu_b), L.ptr(lv_b), L.ptr(eps_b), L.ptr(dl_b), mu_b.numel(), ctx.divisors[1], L.ptr(word), L.ptr(g), L.ptr(dmu_a), L.ptr(dlv_a),
               L.ptr(dmu_b), L.ptr(dlv_b), _stream())
        return dmu_a, dlv_a, dmu_b, dlv_b, None, None, None, None


_SAMPLE_PAIR = True                                             # sample_with_kl of a two-part tuple: one launch each way
_PAIR_MAX = 8192                                                # entries per part (one workgroup of the separate kernels)


def _sample_kl_pair(mu, logvar, beta, batch_size):
    """The two-part tuple through _SampleKlPairFn, or None when the parts are not what it handles."""
    if not (_SAMPLE_PAIR and len(mu) == 2 and all(torch.is_tensor(t) and t.is_cuda for t in (*mu, *logvar))):
        return None
    lay = [_same_layout(m.float(), s.float()) for m, s in zip(mu, logvar)]
    if any(not 1 <= m.numel() <= _PAIR_MAX for m, _, _ in lay):
        return None
    dev = lay[0][0].device
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    capturing = torch.cuda.is_current_stream_capturing()
    if not _NATIVE_RNG or (capturing and (idx not in _noise_epoch or idx not in _noise_base)):
        return None
    keys = (_draw_key(lay[0][0].numel(), idx), _draw_key(lay[1][0].numel(), idx))      # in the order the separate calls draw
    word, beta = beta_word(beta)
    if word is not None:
        divs = [float(batch_size or m.shape[1]) for m in mu]
        l_a, l_b, total = _SampleKlPairDevFn.apply(lay[0][0], lay[0][1], lay[1][0], lay[1][1], word, divs[0], divs[1], keys)
    else:
        scales = [float(beta / (batch_size or m.shape[1])) for m in mu]
        l_a, l_b, total = _SampleKlPairFn.apply(lay[0][0], lay[0][1], lay[1][0], lay[1][1], scales[0], scales[1], keys)
    outs = []
    for l, (_, _, order), m in zip((l_a, l_b), lay, mu):
        outs.append(l.permute([order.index(d) for d in range(m.dim())]) if order is not None else l)
    return tuple(outs), total


def _sample1(mu, logvar):
    m, s, order = _same_layout(mu.float(), logvar.float())
    eps = randn(m.shape, m.device)
    out = _SampleFn.apply(m, s, eps)
    if order is not None:                        # undo the common permutation
        out = out.permute([order.index(d) for d in range(mu.dim())])
    return out


def sample(mu, logvar, model_type=None):
    """l̃ = μ + ε·exp(logσ²/2), ε ~ N(0, 1)  [REF src/models/GOKU.jl:155-163], [REF src/models/LatentODE.jl:82-89]."""
    if isinstance(mu, tuple):
        return tuple(_sample1(m, s) for m, s in zip(mu, logvar))
    return _sample1(mu, logvar)


def _sample_kl1(mu, logvar, scale: float, base, eps=None, word=None):
    """`word`: a β word — `scale` is then the divisor (the batch size) and the kernel forms β ⊘ divisor."""
    m, s, order = _same_layout(mu.float(), logvar.float())
    if eps is None:
        eps = randn(m.shape, m.device)
    else:   # the caller's ε in the layout of μ (tests that compare two runs draw it once)
        eps = eps.float().permute(order) if order is not None else eps.float()
        eps = eps.contiguous()
    if word is not None:
        out, total = _SampleKlDevFn.apply(m, s, eps, word, float(scale), base)
    else:
        out, total = _SampleKlFn.apply(m, s, eps, float(scale), base)
    if order is not None:
        out = out.permute([order.index(d) for d in range(mu.dim())])
    return out, total


def sample_with_kl(mu, logvar, beta: float = 1.0, batch_size=None, eps=None):
    """(l̃, β·kl_loss): `sample(μ, logσ²)` and `β·vector_kl(μ, logσ²)` of the same arguments, computed together (one kernel pass
    each way per part instead of a sample pass, a KL pass and the additions of their cotangents)  [REF src/models/GOKU.jl:155-163],
    [REF src/utils/utils.jl:15-49]. For the GOKU tuple the second part's total continues the first's. `beta`: a number, or a β word
    (module docstring) — the lde_*_dev entry points with divisor = the batch size."""
    word, beta = beta_word(beta)
    if isinstance(mu, tuple):
        if eps is None:
            pair = _sample_kl_pair(mu, logvar, beta if word is None else word, batch_size)
            if pair is not None:
                return pair
        outs, total = [], None
        for i, (m, s) in enumerate(zip(mu, logvar)):
            B = batch_size or m.shape[1]
            o, total = _sample_kl1(m, s, B if word is not None else beta / B, total, None if eps is None else eps[i], word)
            outs.append(o)
        return tuple(outs), total
    B = batch_size or mu.shape[1]
    return _sample_kl1(mu, logvar, B if word is not None else beta / B, None, eps, word)


def _kl_sum(mu, logvar, scale: float):
    m, s, _ = _same_layout(mu.float(), logvar.float())
    return _KlFn.apply(m, s, float(scale))


def vector_kl(mu, logvar, batch_size=None):
    """Σ over entries of kl(μ, logσ²) = (exp(logσ²) + μ² − logσ² − 1)/2, divided by the batch size (the columns; or the global
    `batch_size` when the arrays are one rank's shard); for the GOKU tuple the sum of both parts  [REF src/utils/utils.jl:15-49]."""
    if isinstance(mu, tuple):
        parts = [_kl_sum(m, s, 1.0 / (batch_size or m.shape[1])) for m, s in zip(mu, logvar)]
        out = parts[0]
        for p in parts[1:]:
            out = out + p
        return out
    return _kl_sum(mu, logvar, 1.0 / (batch_size or mu.shape[1]))


def beta_kl(mu, logvar, beta, batch_size=None):
    """β·vector_kl(μ, logσ²) as ONE scalar with β inside the reduction's last kernel. With a β word (module docstring):
    lde_kl_forward_dev — (β ⊘ B)·Σ kl, for the GOKU tuple the second part's total continuing the first's through `base`; the pullback is
    lde_kl_backward_dev. With a number: `beta * vector_kl(...)`, as `loss_batch` has always written it."""
    word, beta = beta_word(beta)
    if word is None:
        return beta * vector_kl(mu, logvar, batch_size)
    total = None
    for m, s in (zip(mu, logvar) if isinstance(mu, tuple) else [(mu, logvar)]):
        mm, ss, _ = _same_layout(m.float(), s.float())
        total = _KlDevFn.apply(mm, ss, word, float(batch_size or m.shape[1]), total)
    return total


def reconstruction_loss(x, x_hat, batch_size=None, plus=None):
    """sum(mean((x − x̂)², dims=(2,3))) for x, x̂ [pixels, B, T]  [REF examples/pendulum_friction-less/model_train.jl:225-238]
    (`batch_size`: the global B when the arrays are one rank's shard). `plus`: a scalar loss term (β·kl_loss from
    `sample_with_kl`) added inside the reduction's last kernel — `reconstruction_loss + β·kl_loss` without elementwise launches."""
    xs, xh, _ = _same_layout(x.float(), x_hat.float())
    n_mean = batch_size or x_hat.shape[1]
    for d in x_hat.shape[2:]:
        n_mean *= d
    if plus is not None:
        return _MseAddFn.apply(xs, xh, 1.0 / n_mean, plus.float())
    return _MseFn.apply(xs, xh, 1.0 / n_mean)


_ONE = {}


def backward(loss: torch.Tensor):
    """loss.backward() with the seed gradient 1 taken from a constant made once per device — `loss.backward()` fills a fresh
    ones_like(loss) every call: one launch per step for a number that never changes."""
    key = (loss.device, loss.dtype)
    one = _ONE.get(key)
    if one is None:
        if loss.is_cuda and torch.cuda.is_current_stream_capturing():
            return loss.backward()
        one = _ONE[key] = torch.ones((), device=loss.device, dtype=loss.dtype)
    loss.backward(gradient=one.expand_as(loss) if loss.dim() else one)

