#!/usr/bin/env python3
"""What the neighbour search costs at the C2 score shape (GPU): python tools/knn_time.py [rows] [reps]

Device time (events on the stream the Session runs on) of Session.knn on `rows` x 50 score-like rows, self-search:
f32 with 15 and 30 neighbours, f64 with 15; beside them the f32-MFMA floor 2 mq mc d_pad FLOP at the data-sheet
157.3 TFLOP/s, and a chunked torch.cdist + topk on the same GPU for the same problem (a yardstick, not code under test).
profiles/knn_time.txt is this script's output."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "single-algebra_amd", "python"))
from sapca import ops  # noqa: E402

PEAK_F32_MFMA = 157.3e12


def scores(rows, d, dtype, seed=0):
    """cluster structure with a decaying spectrum, like the leading principal components of count data"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    scale = 10.0 / torch.arange(1, d + 1, device="cuda", dtype=torch.float64).sqrt()
    centres = torch.randn((40, d), generator=g, device="cuda", dtype=torch.float64) * scale
    which = torch.randint(0, 40, (rows,), generator=g, device="cuda")
    x = centres[which] + 0.35 * scale * torch.randn((rows, d), generator=g, device="cuda", dtype=torch.float64)
    return x.to(dtype).contiguous()


def timed(fn, reps):
    fn()                                                  # warm-up: buffers, code objects
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return sorted(out)


def torch_baseline(x, k, chunk=4096):
    idx = torch.empty((x.shape[0], k), dtype=torch.int64, device=x.device)
    for lo in range(0, x.shape[0], chunk):
        dist = torch.cdist(x[lo:lo + chunk], x)
        dist[torch.arange(dist.shape[0], device=x.device), torch.arange(lo, lo + dist.shape[0], device=x.device)] = float("inf")
        idx[lo:lo + chunk] = dist.topk(k, dim=1, largest=False).indices
    return idx


def main():
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    d = 50
    sess = ops.Session(stream=torch.cuda.current_stream().cuda_stream)
    print(f"knn, self-search on {rows} x {d} score rows, {torch.cuda.get_device_name(0)}; 1 warm-up + {reps} timed calls each")
    print("times: events on the Session's stream around the whole call -- its launches, the gaps between them and its final "
          "stream synchronisation included")
    floor = 2.0 * rows * rows * ((d + 3) // 4 * 4) / PEAK_F32_MFMA * 1e3
    print(f"f32-MFMA floor: 2 mq mc d_pad = {2.0 * rows * rows * ((d + 3) // 4 * 4):.3e} FLOP at 157.3 TFLOP/s = {floor:.2f} ms")
    got = {}
    for dtype, name, ks in ((torch.float32, "f32", (15, 30)), (torch.float64, "f64", (15,))):
        x = scores(rows, d, dtype)
        for k in ks:
            for metric in (("euclidean", "cosine") if (dtype, k) == (torch.float32, 15) else ("euclidean",)):
                t = timed(lambda: got.__setitem__((name, k, metric), sess.knn(x, None, k, metric=metric)), reps)
                print(f"  sapca {name} {metric:9s} n_neighbors {k:3d}: best {t[0]:9.2f} ms, median {t[len(t) // 2]:9.2f} ms"
                      + (f"  ({t[0] / floor:.2f} x the f32 floor)" if name == "f32" else ""))
        if dtype == torch.float32:
            for k in ks:
                t = timed(lambda: got.__setitem__(("torch", k), torch_baseline(x, k)), max(reps - 1, 1))
                print(f"  torch.cdist + topk, f32, chunks of 4096 queries, n_neighbors {k:3d}: best {t[0]:9.2f} ms, median {t[len(t) // 2]:9.2f} ms")
                mine = got[("f32", k, "euclidean")][0].long()
                same = (mine.sort(dim=1).values == got[("torch", k)].sort(dim=1).values).all(dim=1).float().mean().item()
                print(f"    lists with the same members as sapca's: {100.0 * same:.2f} %  (cdist ranks by its own f32 rounding)")


if __name__ == "__main__":
    main()
