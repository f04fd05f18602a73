"""The cases of the Linear launch trace: shared by tests/golden/make_linear_launch_trace.py, which
records them, and tests/test_hip_linear_launch_trace.py, which replays them.

A case is a name and a function that returns the tensors a fixed, seeded call wrote.  ``trace(vsa, rows, fn)`` runs it once to
warm up (weight images, LDS attributes), then once under the torch profiler, and returns the library's device kernel names
in start order and the SHA-256 of the output bytes.  The shapes sit on the edges the pick of csrc/vs_linear_pick.h decides
on: M 128 / 129 (16-bit big tiles), K 256 / 448 / 512 (64-wide k-tiles), M 16128 / 16129 / 16384 / 16385 at N = 1024 (exact
wide tiles and the latency hand-over), N 64 / 256 / 512 (the Linear + LayerNorm kernels).
"""
import hashlib
import math

import torch

SKINNY = (("", -1), ("/tiled", 0))       # VS_SKINNY_ROWS at its default and at 0


def _dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _operands(M, N, K, extra=()):
    g = torch.Generator().manual_seed(7 * M + 3 * N + K)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g)
    more = [torch.randn(*s, generator=g) for s in extra]
    return [t.to(_dev()) for t in [A, W, b] + more]


def _linear(entry, M, N, K, relu, pe):
    def run(vsa):
        lib = vsa._lib.load()
        A, W, b, P = _operands(M, N, K, [(M, N)])
        out = torch.zeros(M, N, device=_dev())
        if entry == "vs_linear_bf16_a16":
            A16 = A.to(torch.bfloat16).contiguous()
            vsa._lib.check(lib.vs_linear_bf16_a16(A16.data_ptr(), W.data_ptr(), b.data_ptr(), out.data_ptr(), M, N, K,
                                                  P.data_ptr() if pe else None, _stream()))
        else:
            vsa._lib.check(getattr(lib, entry)(A.data_ptr(), W.data_ptr(), b.data_ptr(), out.data_ptr(), M, N, K, relu,
                                               P.data_ptr() if pe else None, M if pe else 0, _stream()))
        return [out]
    return run


def _qkv(T):
    def run(vsa):
        lib = vsa._lib.load()
        d, H = 256, 4
        h, W, b = _operands(T, 3 * d, d)
        out = torch.zeros(3, 1, H, T, d // H, device=_dev())
        vsa._lib.check(lib.vs_qkv_proj_f32(h.data_ptr(), W.data_ptr(), b.data_ptr(), out.data_ptr(), 1, T, d, H, _stream()))
        return [out]
    return run


def _res_ln(entry, M, N, K):
    def run(vsa):
        lib = vsa._lib.load()
        A, W, b, res, gam, bet, sw, sb = _operands(M, N, K, [(M, N), (N,), (N,), (1, N), (1,)])
        out, scores = torch.zeros(M, N, device=_dev()), torch.zeros(M, 1, device=_dev())
        vsa._lib.check(getattr(lib, entry)(A.data_ptr(), W.data_ptr(), b.data_ptr(), res.data_ptr(), gam.data_ptr(), bet.data_ptr(),
                                           out.data_ptr(), M, N, K, sw.data_ptr(), sb.data_ptr(), 1, 0, scores.data_ptr(), _stream()))
        return [out, scores]
    return run


def _model(vsa, d, H, L, seed):
    m = vsa.SimNet(num_heads=H, d_model=d, num_layers=L, sparsity=0.0, dropout=0.3)
    m.load_state_dict(vsa.synth.make_state_dict(d, L, seed), strict=True)
    return m.to(_dev())


def _scoring(d, H, B, T, dtype, latency=False):
    made = []

    def run(vsa):
        if not made:                                   # one module per case: the second call finds its weight images packed
            made.append(_model(vsa, d, H, 2, 21).eval().set_compute_dtype(dtype).set_latency_mode(latency))
        m = made[0]
        x = vsa.synth.make_features(B, T, 7, "randn").to(_dev())
        mask = vsa.synth.random_mask(B, T, 5).to(_dev())
        with torch.no_grad():
            logits, hidden = m(x, mask)
        return [logits, hidden]
    return run


def _training(B, T, dtype):
    made = []

    def run(vsa):
        vsa._lib.set_option("VS_TRAIN_LP_MIN_ROWS", 0)
        try:
            if not made:
                made.append(_model(vsa, 256, 4, 2, 23).train().set_train_dtype(dtype))
            m = made[0]
            m.zero_grad(set_to_none=True)
            x = vsa.synth.make_features(B, T, 9, "randn").to(_dev())
            mask = vsa.synth.random_mask(B, T, 3).to(_dev())
            torch.manual_seed(11)                      # the dropout seed is drawn from torch's default CPU generator
            logits, hidden = m(x, mask)
            (logits.square().mean() + 1e-3 * hidden.square().mean()).backward()
            return [logits.detach(), hidden.detach()] + [p.grad for p in m.parameters() if p.grad is not None]
        finally:
            vsa._lib.set_option("VS_TRAIN_LP_MIN_ROWS", -1)
    return run


def cases():
    """[(name, VS_SKINNY_ROWS value, function)] in a fixed order"""
    out = []

    def add(name, fn, settings=SKINNY):
        for suffix, rows in settings:
            out.append((name + suffix, rows, fn))

    # exact fp32: below / at / above the latency hand-over; the first M with 512 wide tiles at N = 1024 and the last without
    for M, N, K, relu, pe in ((100, 256, 256, 0, 0), (100, 256, 256, 0, 1), (16128, 1024, 256, 1, 0), (16129, 1024, 256, 1, 0),
                              (16384, 1024, 256, 1, 0), (16385, 1024, 256, 1, 0), (43776, 384, 256, 0, 0), (2400, 6656, 256, 0, 0)):
        add("vs_linear_f32 M=%d N=%d K=%d relu=%d pe=%d" % (M, N, K, relu, pe), _linear("vs_linear_f32", M, N, K, relu, pe))
    # 16-bit operands: the big-tile edge M 128 / 129 and the 64-wide k-tile edge K 256 / 448 / 512
    for entry in ("vs_linear_bf16", "vs_linear_bf16_a16"):
        for M, N, K, relu, pe in ((128, 256, 512, 0, 0), (129, 256, 512, 0, 0), (129, 256, 448, 0, 0), (128, 256, 256, 0, 0),
                                  (129, 256, 256, 0, 1), (129, 256, 512, 0, 1), (129, 384, 512, 0, 0)):
            add("%s M=%d N=%d K=%d relu=%d pe=%d" % (entry, M, N, K, relu, pe), _linear(entry, M, N, K, relu, pe))
    add("vs_linear_bf16 M=129 N=1024 K=512 relu=1 pe=0", _linear("vs_linear_bf16", 129, 1024, 512, 1, 0))
    for M, N, K, relu, pe in ((128, 256, 256, 0, 0), (129, 256, 256, 0, 0), (129, 1024, 512, 1, 0), (129, 256, 512, 0, 1)):
        add("vs_linear_f16x3 M=%d N=%d K=%d relu=%d pe=%d" % (M, N, K, relu, pe), _linear("vs_linear_f16x3", M, N, K, relu, pe))
    for T in (100, 129):
        add("vs_qkv_proj_f32 T=%d" % T, _qkv(T))
    for prec in ("f32", "bf16", "f16x3"):
        for N in (64, 256, 512):
            add("vs_linear_residual_layernorm_%s M=100 N=%d K=256" % (prec, N),
                _res_ln("vs_linear_residual_layernorm_" + prec, 100, N, 256))
    # whole forwards: M-A in every arithmetic and in latency mode, an M-B-shaped model, a training step
    for dtype in ("fp32", "bf16", "fp16x3"):
        add("scoring M-A B=2 T=150 " + dtype, _scoring(256, 4, 2, 150, dtype))
    add("scoring M-A B=2 T=150 fp32 latency", _scoring(256, 4, 2, 150, "fp32", latency=True), SKINNY[:1])
    for dtype in ("fp32", "bf16"):
        add("scoring M-B d=512 B=1 T=96 " + dtype, _scoring(512, 4, 1, 96, dtype))
    for dtype in ("fp32", "bf16", "fp16"):
        add("training B=2 T=70 " + dtype, _training(2, 70, dtype))
        add("training B=1 T=70 " + dtype, _training(1, 70, dtype), SKINNY[1:])
    return out


def kernel_name(raw):
    """'void (anonymous namespace)::gemm_nt_128<0, 2, 0, 2, 0, 0, 32, 0>(float const*, ...)' -> 'gemm_nt_128<0, 2, 0, 2, 0, 0, 32, 0>'"""
    name = raw.replace("(anonymous namespace)::", "")
    if name.startswith("void "):
        name = name[5:]
    depth = 0
    for i, ch in enumerate(name):
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            return name[:i]
    return name


def trace(vsa, rows, fn):
    """(the library's device kernel names in start order, SHA-256 of the outputs) of one profiled call of ``fn``; a call
    the library refuses is a result too: ([], 'error: ...')"""
    from torch.profiler import ProfilerActivity, profile
    vsa._lib.set_option("VS_SKINNY_ROWS", rows)
    try:
        try:
            fn(vsa)                                       # warm-up: weight images, per-device LDS attributes
        except RuntimeError as exc:
            return [], "error: " + str(exc)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            outs = fn(vsa)
            torch.cuda.synchronize()
    finally:
        vsa._lib.set_option("VS_SKINNY_ROWS", -1)
    events = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    events.sort(key=lambda e: e.time_range.start)
    # torch's own kernels (input set-up, the loss, autograd's accumulations) and copies are not the library's
    names = [kernel_name(e.name) for e in events if "at::" not in e.name and "Memcpy" not in e.name and "Memset" not in e.name]
    digest = hashlib.sha256()
    for t in outs:
        digest.update(t.detach().contiguous().cpu().numpy().tobytes())
    return names, digest.hexdigest()
