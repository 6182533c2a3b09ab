"""MPNet prompt encoder throughput on one GPU: the HIP encode (diffusion_pruning_amd.prompt_encoder, all-mpnet-base-v2 size,
init_synthetic weights; ``encode`` = encoder + masked mean) at (B, L) = (4, 24) -- a handful of pipeline prompts --, (64, 40)
-- the reference's training batch --, (2048, 32) -- one filter_dataset batch -- and (16, 512) -- the longest sequences; ragged
prefix masks (lengths uniform in [L/2, L], sample 0 full): ms per encode and sequences/s, eager and replayed from a HIP
graph (median of --iters replays after warm-up, device events); algorithmic TFLOP/s (prompt_encoder_flops, padded tokens
counted) and share of the bf16 MFMA peak; an A/B of prompt_encoder.BATCH_INVARIANT (the default against launch_policy's own
choice; graph replays timed alternately in this run, graph_ms is the default's best); and a vendor yardstick timed after the
HIP region: the same op sequence as plain bf16 torch modules (hipBLASLt linears, F.scaled_dot_product_attention with the
additive bias + mask), eager and graphed.
--train-json FILE adds the (64, 40) encode's share of a pruning step from a bench.py --config train line of the same session.
Prints ONE JSON line.  usage: python tools/bench_prompt_encoder.py [--iters 20] [--train-json FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

from diffusion_pruning_amd import _lib
from diffusion_pruning_amd import prompt_encoder as P

PEAK_BF16_TFLOPS = 2500.0
SHAPES = ((4, 24), (64, 40), (2048, 32), (16, 512))


def time_events(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g, out


def ragged(B, L, vocab, gen):
    ids = torch.randint(3, vocab, (B, L), generator=gen)
    mask = torch.ones(B, L, dtype=torch.long)
    for i in range(1, B):
        n = int(torch.randint(max(L // 2, 1), L + 1, (1,), generator=gen))
        ids[i, n:] = 1
        mask[i, n:] = 0
    return ids, mask


class VendorEncoder(torch.nn.Module):
    """the same encoder as plain torch ops (bf16): F.embedding, F.linear (hipBLASLt), F.layer_norm, F.gelu and SDPA with
    the additive [B, heads, L, L] bias + mask, then the masked mean in fp32"""

    def __init__(self, sd, cfg):
        super().__init__()
        self.p = {k: v.to(torch.bfloat16) for k, v in sd.items()}
        self.rb = sd["encoder.relative_attention_bias.weight"].float()
        self.cfg = cfg
        self.bias = {}

    def attn_bias(self, L, dev):
        if L not in self.bias:
            t = P.relative_bias_table(self.rb, L).to(dev)
            ar = torch.arange(L, device=dev)
            self.bias[L] = t[:, (ar[None, :] - ar[:, None]) + L - 1].to(torch.bfloat16)[None]
        return self.bias[L]

    def forward(self, ids, mask):
        p, cfg = self.p, self.cfg
        B, L = ids.shape
        C, nh, eps, pad = cfg.hidden_size, cfg.num_attention_heads, cfg.layer_norm_eps, cfg.pad_token_id
        m = ids.ne(pad).int()
        pos = (torch.cumsum(m, 1) * m).long() + pad
        x = p["embeddings.word_embeddings.weight"][ids] + p["embeddings.position_embeddings.weight"][pos]
        x = F.layer_norm(x, (C,), p["embeddings.LayerNorm.weight"], p["embeddings.LayerNorm.bias"], eps)
        am = self.attn_bias(L, ids.device) + ((1.0 - mask.to(torch.bfloat16)) * torch.finfo(torch.bfloat16).min)[:, None, None, :]
        for i in range(cfg.num_hidden_layers):
            pre = f"encoder.layer.{i}."
            lin = lambda t, n: F.linear(t, p[pre + n + ".weight"], p[pre + n + ".bias"])      # noqa: E731
            q, k, v = (lin(x, f"attention.attn.{t}").view(B, L, nh, 64).transpose(1, 2) for t in "qkv")
            o = F.scaled_dot_product_attention(q, k, v, attn_mask=am).transpose(1, 2).reshape(B, L, C)
            x = F.layer_norm(lin(o, "attention.attn.o") + x, (C,), p[pre + "attention.LayerNorm.weight"],
                             p[pre + "attention.LayerNorm.bias"], eps)
            f = lin(F.gelu(lin(x, "intermediate.dense")), "output.dense")
            x = F.layer_norm(f + x, (C,), p[pre + "output.LayerNorm.weight"], p[pre + "output.LayerNorm.bias"], eps)
        mf = mask.float()[..., None]
        return (x.float() * mf).sum(1) / mf.sum(1).clamp(min=1e-9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--train-json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_prompt_encoder: no GPU")
    dev = torch.device("cuda:0")
    _lib.load()
    cfg = P.MPNetConfig()
    m = P.MPNetModel(cfg).init_synthetic(seed=0).to(dev)
    gen = torch.Generator().manual_seed(1)
    data = {s: tuple(t.to(dev) for t in ragged(*s, cfg.vocab_size, gen)) for s in SHAPES}
    res = {"metric": "mpnet_prompt_encode", "model": "all-mpnet-base-v2 MPNetModel (12 layers, 768 wide, 12 heads) + masked mean, bf16",
           "gemm_shapes_tuned": False, "masks": "ragged prefixes, lengths uniform in [L/2, L]", "shapes": {}}
    outs = {}
    with torch.no_grad():
        for s in SHAPES:
            B, L = s
            ids, mask = data[s]
            eager = time_events(lambda: m.encode(ids, mask), a.iters)
            outs[s] = m.encode(ids, mask).clone()
            g, _ = capture(lambda: m.encode(ids, mask))
            ms = time_events(g.replay, a.iters)
            P.BATCH_INVARIANT = False                                        # A/B: launch_policy's own choice (K split at small M)
            m.encode(ids, mask)
            gh, _ = capture(lambda: m.encode(ids, mask))
            P.BATCH_INVARIANT = True
            ab = {1: [], None: []}
            for rep in range(3):
                for sk, gr in (((1, g), (None, gh)) if rep % 2 == 0 else ((None, gh), (1, g))):
                    ab[sk].append(time_events(gr.replay, a.iters))
            ms = min(ms, *ab[1])
            del gh
            flop = P.prompt_encoder_flops(cfg, L) * B
            tf = flop / (ms * 1e-3) / 1e12
            res["shapes"][f"B{B}_L{L}"] = {
                "valid_token_fraction": round(float(mask.float().mean()), 4),
                "graph_ms": round(ms, 4), "sequences_per_s": round(B / (ms * 1e-3), 1),
                "eager_ms": round(eager, 4), "eager_sequences_per_s": round(B / (eager * 1e-3), 1),
                "algorithmic_tflop": round(flop / 1e12, 4), "tflops": round(tf, 1), "frac_of_bf16_peak": round(tf / PEAK_BF16_TFLOPS, 4),
                "batch_invariant_ab": {"invariant_ms": [round(t, 4) for t in ab[1]], "policy_ms": [round(t, 4) for t in ab[None]],
                                       "policy_over_invariant": round(min(ab[None]) / min(ab[1]), 4)}}
            del g
        # ---- vendor yardstick (after the timed HIP region) ---------------------------------------------------------------
        ref = VendorEncoder({k: v.to(dev) for k, v in m.state_dict().items()}, cfg)
        for s in SHAPES:
            B, L = s
            ids, mask = data[s]
            r = res["shapes"][f"B{B}_L{L}"]
            ms = time_events(lambda: ref(ids, mask), a.iters)
            y = ref(ids, mask)
            g, _ = capture(lambda: ref(ids, mask))
            gms = time_events(g.replay, a.iters)
            del g
            r["vendor_eager_ms"], r["vendor_graph_ms"] = round(ms, 4), round(gms, 4)
            r["vendor_graph_over_hip_graph"] = round(gms / r["graph_ms"], 3)
            r["vendor_eager_over_hip_eager"] = round(ms / r["eager_ms"], 3)
            r["rel_l2_vs_vendor"] = float((outs[s] - y).norm() / y.norm())
    if a.train_json:
        with open(a.train_json) as f:
            line = [ln for ln in f.read().splitlines() if ln.startswith("{")][-1]
        step_ms = json.loads(line)["ms_per_step"]
        enc = res["shapes"]["B64_L40"]["eager_ms"]
        res["train_step_bs64"] = {"pruning_step_ms": step_ms, "encode_eager_ms": enc,
                                  "encode_share_of_step_plus_encode": round(enc / (step_ms + enc), 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
