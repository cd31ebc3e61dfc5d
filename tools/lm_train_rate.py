"""Rate of an LM training step (asr_hip/lm_train.py): predicted tokens/s, the split between the sequential part (one launch per
layer and time step, forward and backward) and the token-parallel part (projections, weight gradients, output layer, update), and
for scale the same model's step in fp32 PyTorch on the CPU at 16 threads.

    python tools/lm_train_rate.py [--steps 10] [--warmup 3] [--no-cpu]

Configurations: 2 layers, 64 sentences of 10-40 words; ninp = nhid = 650 with V = 10007, and ninp = nhid = 1024 with V = 32768.
The split is measured with events at both ends of every time loop: a span holds the loop's launches and the gaps between them."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "end2end-asr-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def sentences(n, V, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(2, V, (int(L),), generator=g).tolist() + [0] for L in torch.randint(10, 41, (n,), generator=g)]


def gpu_rate(H, V, steps, warmup):
    from asr_hip.lm_train import LSTMLMTrainer
    tr = LSTMLMTrainer(V, H, H, 2, dropout=0.5, seed=1)
    batch = sentences(64, V, 7)
    ntok = sum(len(s) - 1 for s in batch)
    for _ in range(warmup):
        tr.step(batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step(batch)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / steps
    # one more step with events at the ends of every time loop: a span holds the loop's launches AND the gaps between them
    tr.marks = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    tr.step(batch)
    e1.record()
    torch.cuda.synchronize()
    ev = tr.marks
    tr.marks = None
    seq_ms = sum(a[1].elapsed_time(b[1]) for a, b in zip(ev[0::2], ev[1::2]))
    assert all(a[0] == "seq_begin" and b[0] == "seq_end" for a, b in zip(ev[0::2], ev[1::2]))
    dev_ms = e0.elapsed_time(e1)
    nseq = 2 * tr.nlayers * (max(len(s) for s in batch) - 1)
    return dict(nhid=H, V=V, tokens=ntok, step_ms=wall * 1e3, tokens_per_s=ntok / wall, step_launches=nseq, sequential_ms=seq_ms,
                token_parallel_ms=max(dev_ms - seq_ms, 0.0), step_ms_events=dev_ms)


def cpu_rate(H, V, steps):
    torch.set_num_threads(16)
    batch = sorted(sentences(64, V, 7), key=lambda s: -len(s))
    ntok = sum(len(s) - 1 for s in batch)
    emb, rnn, dec = torch.nn.Embedding(V, H), torch.nn.LSTM(H, H, 2, dropout=0.5), torch.nn.Linear(H, V)
    params = list(emb.parameters()) + list(rnn.parameters()) + list(dec.parameters())
    opt = torch.optim.Adam(params, lr=1e-3)
    from torch.nn.utils.rnn import pack_sequence

    def step():
        opt.zero_grad()
        pk = pack_sequence([emb(torch.tensor(s[:-1])) for s in batch], enforce_sorted=True)
        tgt = pack_sequence([torch.tensor(s[1:]) for s in batch], enforce_sorted=True).data
        loss = torch.nn.functional.cross_entropy(dec(rnn(pk)[0].data), tgt)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 0.25)
        opt.step()
    step()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    wall = (time.perf_counter() - t0) / steps
    return dict(nhid=H, V=V, tokens=ntok, cpu_step_ms=wall * 1e3, cpu_tokens_per_s=ntok / wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    for H, V in ((650, 10007), (1024, 32768)):
        r = gpu_rate(H, V, a.steps, a.warmup)
        print("gpu  nhid %4d V %5d: %d tokens/step  %.2f ms/step  %.0f tokens/s | %d step launches %.2f ms (%.0f%%), token-parallel "
              "%.2f ms" % (r["nhid"], r["V"], r["tokens"], r["step_ms"], r["tokens_per_s"], r["step_launches"], r["sequential_ms"],
                           100 * r["sequential_ms"] / max(r["step_ms_events"], 1e-9), r["token_parallel_ms"]), flush=True)
        if not a.no_cpu:
            c = cpu_rate(H, V, max(1, a.steps // 5))
            print("cpu  nhid %4d V %5d: %.1f ms/step  %.0f tokens/s (fp32 PyTorch, 16 threads)" % (c["nhid"], c["V"], c["cpu_step_ms"],
                                                                                                  c["cpu_tokens_per_s"]), flush=True)


if __name__ == "__main__":
    main()
