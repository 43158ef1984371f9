#!/usr/bin/env python3
"""One-op probes behind `csrc/optim_adam.hip`: how does each foreach op of `torch.optim.adam._multi_tensor_adam` round on this GPU?

  python tools/adam_probe.py > profiles/adam/rounding_probe.txt

Every op is run on 2^20 random elements (gradients and moments at magnitude 1, then 1e-3) and compared with candidate formulas:
one rounding (a fused multiply-add, evaluated in fp64 and rounded to fp32 once), every operation rounded on its own, a reciprocal in
place of a division, scalars cast to fp32 or left as doubles. Each line prints, per candidate, the number of elements whose bits
differ from the torch op; the candidate with 0 is what the kernel computes. The last block asks whether the ops keep fp32 denormals.
Needs a GPU and PyTorch only (not this package)."""
import numpy as np
import torch

torch.manual_seed(0)
N = 1 << 20
dev = "cuda"


def r(scale=1.0):
    return (torch.randn(N, device=dev) * scale).float()


def f32(x):
    return float(np.float32(x))


def mism(name, got, **cands):
    out = []
    for k, v in cands.items():
        v = v.float()
        bad = int(((got != v) & ~(got.isnan() & v.isnan())).sum())
        out.append(f"{k}={bad}")
    print(f"{name}: " + " ".join(out), flush=True)


def d(x):
    return x.double()


print(torch.__version__, torch.cuda.get_device_name(0))
for scale in (1.0, 1e-3):
    print("--- scale", scale)
    g, p, m = r(scale), r(), r(scale)
    v = r(scale).square()
    # 2b add(alpha)
    wd = 5e-4
    got = torch._foreach_add([g, g.clone()], [p, p.clone()], alpha=wd)[0]
    mism("2b add alpha", got, fused=d(g) + d(p) * f32(wd), twice=g + p * f32(wd), fused_dblalpha=d(g) + d(p) * wd)
    # 3 lerp
    for beta1 in (0.9, 0.937, 0.4, 0.5):
        w = 1 - beta1
        ms = [m.clone(), m.clone()]
        torch._foreach_lerp_(ms, [g, g.clone()], w)
        got = ms[0]
        diff = g - m
        w32 = f32(w)
        if w32 < 0.5:
            mism(f"3 lerp w={w32!r} small", got, fused=d(m) + w32 * d(diff), twice=m + diff * w32, fused_dblw=d(m) + w * d(diff),
                 onefma_nodiffround=d(m) + w32 * (d(g) - d(m)))
        else:
            omw = f32(np.float32(1) - np.float32(w32))
            mism(f"3 lerp w={w32!r} large omw={omw!r}", got, fused=d(g) - d(diff) * omw, twice=g - diff * omw,
                 fused_dblomw=d(g) - d(diff) * (1.0 - w), small_branch_fused=d(m) + w32 * d(diff))
    # 4 mul
    vs = [v.clone(), v.clone()]
    torch._foreach_mul_(vs, 0.999)
    mism("4 mul beta2", vs[0], f32=v * f32(0.999), dbl=d(v) * 0.999)
    # 5 addcmul
    for beta2 in (0.999, 0.9):
        value = 1 - beta2
        v32 = f32(value)
        vs = [v.clone(), v.clone()]
        torch._foreach_addcmul_(vs, [g, g.clone()], [g, g.clone()], value)
        gg = g * g
        mism(f"5 addcmul value={v32!r}", vs[0], A_fma_val_gg=d(v) + v32 * d(gg), B_all_sep=v + (gg * v32), C_fma_valg_g=d(v) + d(g * v32) * d(g),
             D_one_round=d(v) + v32 * d(g) * d(g), E_sep_valg_g=v + (g * v32) * g)
    # 6 sqrt
    got = torch._foreach_sqrt([v, v.clone()])[0]
    mism("6 sqrt", got, correct=d(v).sqrt())
    # 7 div by a scalar list
    dd = got
    for s in (0.0316227766016838, 0.31606961258558215, 0.9999):
        xs = [dd.clone(), dd.clone()]
        torch._foreach_div_(xs, [s, s])
        mism(f"7 div s={s!r}", xs[0], true_f32s=d(dd) / f32(s), true_dbls=d(dd) / s, recip_f32=dd * f32(np.float32(1) / np.float32(s)),
             recip_dbl=dd * f32(1.0 / s), recip_dbl_exactmul=d(dd) * (1.0 / s))
    # 8 add eps
    xs = [dd.clone(), dd.clone()]
    torch._foreach_add_(xs, 1e-8)
    mism("8 add eps", xs[0], f32=dd + f32(1e-8), dbl=d(dd) + 1e-8)
    den = xs[0] + f32(1e-3) * scale
    # 9 addcdiv with a scalar list
    for step in (-0.01, -0.0003162):
        s32 = f32(step)
        ps = [p.clone(), p.clone()]
        torch._foreach_addcdiv_(ps, [m, m.clone()], [den, den.clone()], [step, step])
        q = (d(m) / d(den)).float()
        rc = (1.0 / d(den)).float()
        mism(f"9 addcdiv step={s32!r}", ps[0], A_fma_step_q=d(p) + s32 * d(q), B_sep=p + q * s32, C_recip_fma=d(p) + s32 * d(m * rc),
             D_one_round=d(p) + s32 * d(m) / d(den), E_stepm_over_d=d(p) + d(m * s32) / d(den), F_fma_dblstep=d(p) + step * d(q))

print("--- denormals")
tiny = torch.full((N,), 1e-20, device=dev)
print("plain mul 1e-20*1e-20:", float((tiny * tiny)[0]))
vs = [torch.zeros(N, device=dev), torch.zeros(N, device=dev)]
torch._foreach_addcmul_(vs, [tiny, tiny.clone()], [tiny, tiny.clone()], 1 - 0.999)
print("addcmul 0 + 1e-3*(1e-20)^2:", float(vs[0][0]), " expected (denormals kept)", float(np.float32(np.float32(1e-20) * np.float32(1e-20)) * np.float32(1 - 0.999)))
den_in = torch.full((N,), 1e-40, device=dev)
print("denormal input as stored:", float(den_in[0]))
print("foreach_mul denormal*0.999:", float(torch._foreach_mul([den_in], 0.999)[0][0]))
print("foreach_sqrt(1e-40):", float(torch._foreach_sqrt([den_in])[0][0]), "want", float(np.sqrt(np.float32(1e-40))))
ms = [torch.zeros(N, device=dev)]
torch._foreach_lerp_(ms, [den_in], 0.1)
print("lerp(0, 1e-40, 0.1):", float(ms[0][0]))
xs = [den_in.clone()]
torch._foreach_div_(xs, [0.5])
print("div denormal / 0.5:", float(xs[0][0]))
ps = [torch.zeros(N, device=dev)]
torch._foreach_addcdiv_(ps, [den_in], [torch.ones(N, device=dev)], [-0.5])
print("addcdiv 0 + -0.5 * (1e-40/1):", float(ps[0][0]))
xs = torch._foreach_add([den_in], [den_in], alpha=0.5)
print("add alpha denormal:", float(xs[0][0]))
# full-chain sanity: torch AdamW foreach with 1e-20 grads
q = torch.nn.Parameter(torch.ones(8, device=dev))
o = torch.optim.AdamW([q], lr=1e-3, foreach=True)
q.grad = torch.full((8,), 1e-20, device=dev)
o.step()
print("AdamW after 1e-20 grad: exp_avg_sq", float(o.state[q]["exp_avg_sq"][0]), "exp_avg", float(o.state[q]["exp_avg"][0]), "p", repr(float(q[0])))
print("PROBE DONE")
