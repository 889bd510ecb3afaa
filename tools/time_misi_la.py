"""Time online MISI on the device: misi_la_dev (k_misi_la of lws_gla.hip; look-ahead 3, 5 iterations, no signals) on 64 mixtures of
K = 2 and K = 4 sources, alternating with (a) rtisi_la_dev on the same B K spectrograms -- the same transforms with K times the
workgroups in flight and no coupling: the yardstick, not an alternative (it ignores the mixture).  (b) On a short clip the same
iteration is composed from the public pieces (istft_dev -> torch -> stft_dev per inner step), which is what a caller had before; the
composition must agree with the kernel.  (c) rtisi_la_dev on the 256 x 628 stack of tools/time_rtisi.py, to compare with the figure
recorded before k_misi_la joined its translation unit.  HIP events around each call, after a warm-up; medians and the spread over
`--reps` alternating repetitions.
    PYTHONPATH=. python tools/time_misi_la.py [--reps 9 --out profiles/misi_la_iteration.json]"""
import argparse, json
import numpy as np, torch
import lws_amd

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--look-ahead", type=int, default=3)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--clip", type=int, default=24, help="frames of the short clip the composition is timed on (0: skip it)")
ap.add_argument("--out", default=None)
ap.add_argument("--small", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("time_misi_la.py needs a GPU")
# (fsize, fshift, B, T, K)
SHAPES = [(512, 128, 64, 500, 2), (512, 128, 64, 500, 4)] if not a.small else [(64, 16, 3, 12, 2)]
RTISI = (512, 128, 256, 628) if not a.small else (64, 16, 3, 12)
RTISI_BEFORE_MS = 60.06                          # rtisi_la_dev on that stack before this kernel existed
LA, n = a.look_ahead, a.iters


def composed(p, c0, A, y):
    """misi_la from the public calls, on the uncut timeline (the cuts of perfectrec as a mask); returns c."""
    N, hop = p.fsize, p.fshift
    B, K, T, F = c0.shape
    c = c0.clone()
    total = hop * (T - 1) + N
    keep = torch.ones(total, device=c.device)
    lo = 0
    if p.perfectrec:
        lo = N - hop if N % hop == 0 else N - N % hop
        keep[:lo] = 0
        keep[total - (N - hop):] = 0
    yfull = torch.zeros((B, total), device=c.device)
    yfull[:, lo:lo + y.shape[1]] = y
    w = torch.as_tensor(p.awin * p.swin, dtype=torch.float32, device=c.device)
    num = torch.zeros((T, total), device=c.device)                       # num[l]: the weight of the frames 0 .. l
    for j in range(T):
        num[j:, hop * j: hop * j + N] += w
    g = torch.where(num[-1] != 0, num / num[-1].clamp_min(1e-30), torch.ones_like(num))
    done = torch.zeros((B, K, total), device=c.device)
    for m in range(T):
        last = min(m + LA, T - 1)
        a0, a1 = hop * m, hop * last + N
        target = keep[a0:a1] * g[last, a0:a1] * yfull[:, a0:a1]
        for it in range(n):
            f = lws_amd.istft_dev(c[:, :, m:last + 1].reshape(B * K, last + 1 - m, F), hop, p.swin, perfectrec=False)
            yk = (done[:, :, a0:a1] + f.reshape(B, K, -1)) * keep[a0:a1]
            x = yk + ((target - yk.sum(dim=1)) / K)[:, None]
            X = lws_amd.stft_dev(x.reshape(B * K, -1), N, hop, p.awin, perfectrec=False).reshape(B, K, last + 1 - m, F)
            c[:, :, m:last + 1] = X * (A[:, :, m:last + 1] / X.abs())    # (no zero bins in these inputs)
        done[:, :, a0:a0 + N] += lws_amd.istft_dev(c[:, :, m].reshape(B * K, 1, F), hop, p.swin, perfectrec=False).reshape(B, K, N)
    return c


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(v, transforms):
    return {"median_ms": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)),
            "median_ns_per_frame_transform": float(np.median(v)) * 1e6 / transforms}


def alternate(runs):
    for _ in range(a.warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, fn in runs.items():
            ms[k].append(timed(fn))
    return ms


def transforms_of(B, T):
    """Forward and inverse transforms of one frame: n (LA + 1) of each per frame, less the look-aheads the end cuts short."""
    return 2 * B * n * sum(min(m + LA, T - 1) - m + 1 for m in range(T))


results = []
for fsize, fshift, B, T, K in SHAPES:
    F = fsize // 2 + 1
    p = lws_amd.lws(fsize, fshift)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    level = torch.tensor([1.0, 0.3, 3.0, 1.0], device="cuda")[:K]
    x = torch.randn((B, K, lws_amd._capi.istft_length(T, fsize, fshift, True)), device="cuda", generator=g) * level[None, :, None]
    y = x.sum(dim=1)
    X = p.stft_dev(x.reshape(B * K, -1)).reshape(B, K, T, F)
    c0 = X * torch.polar(torch.ones_like(X.real), 0.3 * torch.randn(X.shape, device="cuda", generator=g))
    A = X.abs()
    flat, Aflat = c0.reshape(B * K, T, F), A.reshape(B * K, T, F)
    ms = alternate({"misi_la": lambda: p.misi_la_dev(c0, y, n, look_ahead=LA, magnitudes=A),
                    "rtisi_la": lambda: p.rtisi_la_dev(flat, n, look_ahead=LA, magnitudes=Aflat)})
    row = {"fsize": fsize, "fshift": fshift, "B": B, "K": K, "T": T, "iterations": n, "look_ahead": LA, "reps": a.reps,
           "misi_la": stats(ms["misi_la"], transforms_of(B * K, T)), "rtisi_la": stats(ms["rtisi_la"], transforms_of(B * K, T))}
    row["misi_la_over_rtisi_la_of_medians"] = row["misi_la"]["median_ms"] / row["rtisi_la"]["median_ms"]
    if a.clip:
        Tc = min(a.clip, T)
        cc, Ac = c0[:, :, :Tc].contiguous(), A[:, :, :Tc].contiguous()
        yc = y[:, :lws_amd._capi.istft_length(Tc, fsize, fshift, True)].contiguous()
        short = {"misi_la": lambda: p.misi_la_dev(cc, yc, n, look_ahead=LA, magnitudes=Ac), "composed": lambda: composed(p, cc, Ac, yc)}
        d = short["misi_la"]() - short["composed"]()
        row["clip"] = {"T": Tc, "rel_l2_kernel_vs_composed": float(torch.linalg.vector_norm(d) / torch.linalg.vector_norm(cc))}
        cms = alternate(short)
        for k, v in cms.items():
            row["clip"][k] = stats(v, transforms_of(B * K, Tc))
        row["clip"]["speedup_of_medians"] = row["clip"]["composed"]["median_ms"] / row["clip"]["misi_la"]["median_ms"]
    results.append(row)
    print(json.dumps(row), flush=True)

fsize, fshift, B, T = RTISI
p = lws_amd.lws(fsize, fshift)
g = torch.Generator(device="cuda"); g.manual_seed(1)
X = p.stft_dev(torch.randn((B, lws_amd._capi.istft_length(T, fsize, fshift, True)), device="cuda", generator=g))
c0 = X * torch.polar(torch.ones_like(X.real), 0.3 * torch.randn(X.shape, device="cuda", generator=g))
A = X.abs()
ms = alternate({"rtisi_la": lambda: p.rtisi_la_dev(c0, n, look_ahead=LA, magnitudes=A)})
unchanged = {"fsize": fsize, "fshift": fshift, "B": B, "T": T, "iterations": n, "look_ahead": LA, "reps": a.reps,
             "rtisi_la": stats(ms["rtisi_la"], transforms_of(B, T)), "recorded_before_ms": RTISI_BEFORE_MS}
unchanged["ratio_to_recorded"] = unchanged["rtisi_la"]["median_ms"] / RTISI_BEFORE_MS
print(json.dumps(unchanged), flush=True)
if a.out:
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": results, "rtisi_la_unchanged": unchanged}, f, indent=1)
        f.write("\n")
