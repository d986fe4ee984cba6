"""The LARS / LAMB math contract of optim/fused.py, transcribed in float64: the oracle of
test_layerwise_optim_cpu.py and test_layerwise_optim_gpu.py."""
import torch

SHAPES = [(64, 3, 7, 7), (64,), (1000, 2048), (3,), (70001,), (5, 5)]  # test_kernels_gpu.py's optimizer set
TOL = dict(rtol=1e-5, atol=1e-6)  # the project's fused-vs-torch optimizer tolerance


def lars_oracle(ws, grads, lr, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False,
                trust_coefficient=0.001, eps=1e-8, adapt=True, maximize=False):
    ws = [w.detach().double().clone() for w in ws]
    bufs = [None] * len(ws)
    ratios = []
    for gs in grads:
        ratios.append([])
        for i, g in enumerate(gs):
            w, g = ws[i], (-g if maximize else g).double()
            wn, gn = w.norm(), g.norm()
            r = trust_coefficient * wn / (gn + weight_decay * wn + eps) if adapt and wn > 0 and gn > 0 else 1.0
            ratios[-1].append(float(r))
            d = r * (g + weight_decay * w)
            if momentum != 0:
                bufs[i] = d.clone() if bufs[i] is None else momentum * bufs[i] + (1 - dampening) * d
                d = d + momentum * bufs[i] if nesterov else bufs[i]
            ws[i] = w - lr * d
    return ws, ratios


def lamb_oracle(ws, grads, lr, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, adapt=True, maximize=False):
    ws = [w.detach().double().clone() for w in ws]
    ms = [torch.zeros_like(w) for w in ws]
    vs = [torch.zeros_like(w) for w in ws]
    b1, b2 = betas
    ratios = []
    for t, gs in enumerate(grads, start=1):
        ratios.append([])
        for i, g in enumerate(gs):
            w, g = ws[i], (-g if maximize else g).double()
            ms[i] = ms[i] + (1 - b1) * (g - ms[i])
            vs[i] = b2 * vs[i] + (1 - b2) * g * g
            u = (ms[i] / (1 - b1 ** t)) / ((vs[i] / (1 - b2 ** t)).sqrt() + eps) + weight_decay * w
            wn, un = w.norm(), u.norm()
            r = wn / un if adapt and wn > 0 and un > 0 else 1.0
            ratios[-1].append(float(r))
            ws[i] = w - lr * r * u
    return ws, ratios
