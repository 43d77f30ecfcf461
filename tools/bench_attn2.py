#!/usr/bin/env python3
"""attention_f16x2.hip stand-alone: error against float64 attention and time per launch at the encoder's self-attention shape
(B = 64, T = 512 padded from 500, 4 heads of 128) and at the decoder's cross-attention shape, for every schedule the loaded library
has (3 = the product's; 0 / 1 in the measurement library). PF_LIB_PATH picks the library (funasr_amd/_lib.py), so two builds can
alternate in one job, each in a fresh process:

    PF_LIB_PATH=/path/to/parent/libparaformer_hip.so python tools/bench_attn2.py --label parent --out /tmp/attn2.jsonl
    python tools/bench_attn2.py --label branch --out /tmp/attn2.jsonl

One JSON line per shape on stdout (and appended to --out). --dump FILE saves the self-attention output of the first four sequences
(variant 3); `bench_attn2.py bits A B` then counts the elements in which two such files differ."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

SHAPES = (("self", 64, 512, 512, 500), ("cross", 64, 230, 512, 500))


def bits(a_path, b_path):
    a, b = torch.load(a_path), torch.load(b_path)
    d = (a["o"].double() - b["o"].double()).abs()
    row = {"mode": "bits", "a": a["label"], "b": b["label"], "elements": d.numel(), "differ": int((d > 0).sum()), "max_abs_diff": float(d.max()),
           "max_abs_o": float(a["o"].abs().max()), "err_f64_a": a["err"], "err_f64_b": b["err"]}
    print(json.dumps(row), flush=True)
    return row


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "bits":
        bits(sys.argv[2], sys.argv[3])
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default=os.environ.get("PF_LIB_PATH") and "PF_LIB_PATH" or "product")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--dump", default=None, help="save the self-attention output (first four sequences, variant 3) for `bits`")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    from funasr_amd import _lib, ops
    variants = (0, 1, 3) if _lib.load().pf_measurement_build() else (3,)
    dev = torch.device("cuda:0")
    scale = 128 ** -0.5
    for name, B, Tq, Tp, klen in SHAPES:
        g = torch.Generator().manual_seed(0)
        q, k, v = (torch.randn(B, T, 512, generator=g).to(dev) for T in (Tq, Tp, Tp))
        klens = torch.full((B,), klen, dtype=torch.int32, device=dev)
        klens[1] = 37; klens[2] = 1
        qq, kk, vv = (t[:4].double().view(4, -1, 4, 128).transpose(1, 2) for t in (q, k, v))
        mask = torch.arange(Tp, device=dev)[None, None, None, :] >= klens[:4, None, None, None]
        sc = ((qq * scale) @ kk.transpose(-1, -2)).masked_fill(mask, -float("inf"))
        ref = (torch.softmax(sc, -1).masked_fill(mask, 0) @ vv).transpose(1, 2).reshape(4, Tq, 512)
        row = {"lib": args.label, "shape": name, "B": B, "Tq": Tq, "Tp": Tp, "klen": klen}
        outs = {}
        for variant in variants:
            outs[variant] = ops.attention_f16x2(q, k, v, klens, 4, scale, variant=variant)
            row[f"err_v{variant}"] = float((outs[variant][:4].double() - ref).abs().max())
            us = [ops.attention_f16x2(q, k, v, klens, 4, scale, variant=variant, time_iters=args.iters)[1] * 1e3 for _ in range(args.rounds)]
            row[f"us_v{variant}"] = round(min(us), 2)
            row[f"us_v{variant}_rounds"] = [round(x, 2) for x in us]
        if 0 in outs:
            row["v0_bitwise_equal_v1"] = bool(torch.equal(outs[0], outs[1]))
        row["tflops_eq_v3"] = round(4.0 * sum(int(x) for x in klens.tolist()) * Tq * 512 / row["us_v3"] / 1e6, 1)
        print(json.dumps(row), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(row) + "\n")
        if args.dump and name == "self":
            torch.save({"label": args.label, "o": outs[3][:4].cpu(), "err": row["err_v3"]}, args.dump)


if __name__ == "__main__":
    main()
