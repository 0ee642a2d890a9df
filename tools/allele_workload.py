"""The library of tools/bench_bubbles.py and tools/bench_unitigs.py: synth.torch_workload's transcriptome and sampling, resident in HBM,
with a substitution allele in one transcript of `every`."""
import torch

from soapdenovo_trans_amd import synth


def workload_with_alleles(n_reads, read_len, T, device, K, every, seed=42, err=0.002, chunk=1 << 20):
    """synth.torch_workload, read for read (same generator, same draws), and then: transcript t with t % every == 0 has a site in its
    middle, and a read that covers it carries (base + 1) & 3 there with probability 1/2 (a generator of its own, so that nothing else
    moves).  Returns (words, offsets, nwords, sites planted)"""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    g2 = torch.Generator(device=device)
    g2.manual_seed(seed + 1)
    codes_np, starts_np, w_np = synth.make_transcriptome(T, seed=42, sigma=2.0)
    tx = torch.from_numpy(codes_np).to(device)
    starts = torch.from_numpy(starts_np).to(device)
    lens_t = starts[1:] - starts[:-1]
    site = starts[:-1] + lens_t // 2
    planted = (torch.arange(T, device=device) % every == 0) & (lens_t >= 2 * K + 2)
    cdf = torch.cumsum(torch.from_numpy(w_np).to(device=device, dtype=torch.float32).double(), 0)
    cdf = cdf / cdf[-1]
    nwords = (n_reads * read_len + 15) // 16 + 4
    words = torch.zeros(nwords, dtype=torch.int32, device=device)
    chunk = max(16, chunk // 16 * 16)
    shifts = (30 - 2 * torch.arange(16, device=device, dtype=torch.int64))
    ar = torch.arange(read_len, device=device, dtype=torch.int64)
    for c0 in range(0, n_reads, chunk):
        m = min(chunk, n_reads - c0)
        u = torch.rand(m, generator=g, device=device, dtype=torch.float64)
        t = torch.searchsorted(cdf, u).clamp_(max=T - 1)
        span = (lens_t[t] - read_len + 1).clamp_(min=1)
        pos = (torch.rand(m, generator=g, device=device, dtype=torch.float64) * span).long() + starts[t]
        flip = torch.rand(m, generator=g, device=device) < 0.5
        idx = torch.where(flip[:, None], pos[:, None] + (read_len - 1 - ar)[None, :], pos[:, None] + ar[None, :])
        rc = tx[idx]
        other = (torch.rand(m, generator=g2, device=device) < 0.5) & planted[t]
        rc = torch.where(other[:, None] & (idx == site[t][:, None]), (rc + 1) & 3, rc)
        rc = torch.where(flip[:, None], rc ^ 2, rc)
        if err > 0:
            e = torch.rand(rc.shape, generator=g, device=device) < err
            sub = torch.randint(1, 4, rc.shape, generator=g, device=device, dtype=torch.uint8)
            rc = torch.where(e, (rc + sub) & 3, rc)
        flat = rc.reshape(-1).long()
        pad = (-flat.numel()) % 16
        if pad:
            flat = torch.cat([flat, torch.zeros(pad, dtype=torch.int64, device=device)])
        w = (flat.view(-1, 16) << shifts).sum(dim=1)
        w = torch.where(w >= (1 << 31), w - (1 << 32), w).to(torch.int32)
        w0 = (c0 * read_len) // 16
        words[w0:w0 + w.numel()] = w
        del idx, rc, flat, w
    offsets = torch.arange(n_reads + 1, device=device, dtype=torch.int64) * read_len
    return words, offsets, nwords, int(planted.sum())
