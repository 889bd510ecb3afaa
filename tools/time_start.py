"""Time one push of one frame into the look-ahead streams in their steady state, per start (lws(512,128), look-ahead 3, 5 iterations,
explicit magnitudes, no signal): RtisiLaStream at B = 1 and B = 256 under start='given' and 'overlap', MisiLaStream with K = 2 at B = 1
and B = 64 under 'given' and 'mixture'.  HIP events around `--pushes` consecutive pushes after `--warmup` of them, so the figure is the
device time of a push as a real-time caller strings them together; `--reps` repetitions, the starts alternating; every start is pushed
the same tensors (complex rows and their magnitudes: the magnitude-only starts do not read the rows), so the host side of a push is the
same.  --starts given times the default alone and passes no keyword, so that the script also runs against a tree that has none.
    PYTHONPATH=. python tools/time_start.py [--reps 3 --out profiles/start_push.json]"""
import argparse, json
import numpy as np, torch
import lws_amd

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--look-ahead", type=int, default=3)
ap.add_argument("--pushes", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--starts", default="all", choices=["all", "given"])
ap.add_argument("--out", default=None)
ap.add_argument("--small", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("time_start.py needs a GPU")
fsize, fshift, RB, MB, K = (512, 128, [1, 256], [1, 64], 2) if not a.small else (64, 16, [1, 3], [1, 2], 2)
LA, n = a.look_ahead, a.iters
T = LA + 1 + a.warmup + a.pushes
F = fsize // 2 + 1
p = lws_amd.lws(fsize, fshift)
g = torch.Generator(device="cuda"); g.manual_seed(1)
B = max(RB + MB)
x = torch.randn((B, K, fshift * (T - 1) + fsize), device="cuda", generator=g)
X = p.stft_dev(x.reshape(B * K, -1)).reshape(B, K, -1, F)[:, :, :T]
c0 = (X * torch.polar(torch.ones_like(X.real), 0.3 * torch.randn(X.shape, device="cuda", generator=g))).contiguous()
A = X.abs().contiguous()
y = x.sum(dim=1).contiguous()


def kw(start):
    return {} if start == "given" else {"start": start}


def rtisi(b, start):
    s = p.rtisi_la_stream(n, look_ahead=LA, batch=b, **kw(start))
    rows = [(c0[:b, 0, m:m + 1].contiguous(), A[:b, 0, m:m + 1].contiguous()) for m in range(T)]
    return s, [lambda r=r: s.push(r[0], r[1]) for r in rows]


def misi(b, start):
    s = p.misi_la_stream(K, n, look_ahead=LA, batch=b, **kw(start))
    calls, at = [], 0
    for m in range(T):
        ns = s._need(m + 1) - s._need(m)            # what samples_needed(1) will say at this push
        r = (c0[:b, :, m:m + 1].contiguous(), y[:b, at:at + ns].contiguous(), A[:b, :, m:m + 1].contiguous())
        at += ns
        calls.append(lambda r=r: s.push(r[0], r[1], r[2]))
    return s, calls


def one(make, b, start):
    s, calls = make(b, start)
    for c in calls[:LA + 1 + a.warmup]:
        c()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for c in calls[LA + 1 + a.warmup:]:
        c()
    e1.record()
    e1.synchronize()
    s.finish()
    s.close()
    return 1e3 * e0.elapsed_time(e1) / a.pushes      # microseconds per push


cases = [("rtisi", rtisi, b, ["given", "overlap"]) for b in RB] + [("misi_K%d" % K, misi, b, ["given", "mixture"]) for b in MB]
result = {"fsize": fsize, "fshift": fshift, "iterations": n, "look_ahead": LA, "pushes": a.pushes, "warmup": a.warmup, "reps": a.reps,
          "push_us": {}}
for name, make, b, starts in cases:
    starts = starts[:1] if a.starts == "given" else starts
    us = {s: [] for s in starts}
    for s in starts:                                 # once, untimed: allocations, windows, the kernels' first launch
        one(make, b, s)
    for _ in range(a.reps):                          # alternate them
        for s in starts:
            us[s].append(one(make, b, s))
    row = {s: {"runs_us": v, "median_us": float(np.median(v))} for s, v in us.items()}
    for s in starts[1:]:
        row[s]["over_given_of_medians"] = row[s]["median_us"] / row["given"]["median_us"]
    result["push_us"]["%s_B%d" % (name, b)] = row
print(json.dumps(result), flush=True)
if a.out:
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": [result]}, f, indent=1)
        f.write("\n")
