#!/usr/bin/env python3
"""Generate tests/golden/launch_traces.json.gz: the launch sequences (tests/launch_trace.py) that ppt_amd.engine.vit_block_forward
and text_tower_forward / text_tower_backward produce over a grid of shapes, precisions and switch settings.  No GPU needed.

    python tests/golden/make_golden_traces.py

The file holds the commit it was recorded at, the cases -- each with the SHA-1 of its trace and an index into the distinct trace
texts -- and the distinct texts, once each.  It pins WHAT IS LAUNCHED: regenerate it only with a change that means to launch
something else, and say so there.  A run that reproduces the recorded traces leaves the file (and its commit) as it is.

ViT block (D = 384, 6 heads, Tn = 129): B on both sides of every row threshold of the block (8 192, 16 000, 24 576 rows) and 1,
three operand dtypes, saving or not, pos_in_x, add_pos_out, DropPath factors or none, fc1 1536 / 768 wide -- the full product at the
default switches; every switch setting over the axes that choose a kernel (rows, fp32 / fp16, saving, pos_in_x, fc1 width).
Text tower (Wd = 512, 8 heads, 3 prompts of 8 tokens): eff_len, shared prefix, prompts / rows_in, 1 / 3 layers, saving or not, c_fc
2048 / 1024 wide, four operand forms -- all inputs at the default switches, two of them (plain prompts; truncated, prefix-shared
rows_in) under every switch setting, under per-half stage precisions and a gradient scale; 17 x 241 = 4 097 rows (split-K off).
Asserted: every kernel choice the engine can make appears in at least one case (COVER).
"""
import gzip
import hashlib
import itertools
import json
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import launch_trace as LT                     # noqa: E402

OUT = os.path.join(HERE, "launch_traces.json.gz")

BLOCK_SWITCHES = [
    {}, {"FUSED_MLP": False}, {"FUSED_PROJ": False}, {"ROWGEMM_MIN_ROWS": 0}, {"ROWGEMM_MIN_ROWS": 1 << 30}, {"LNLIN_MAX_ROWS": 0},
    {"BLOCK_PATH": {"qkv": "v2", "proj": "v2", "mlp": "v2"}},
    {"BLOCK_PATH": {"qkv": "rowgemm", "proj": "rowgemm", "mlp": "rowgemm"}},
    {"BLOCK_PATH": {"qkv": "auto", "proj": "fused", "mlp": "rowgemm"}},
    {"BLOCK_PATH": {"qkv": "auto", "proj": "rowgemm", "mlp": "fused"}}]
TEXT_SWITCHES = [
    {}, {"TEXT_FUSE_LN": True}, {"TEXT_SPLITK": False}, {"TEXT_MLP_PAIR": False}, {"TEXT_MLP_PAIR_LN": False},
    {"TEXT_MLP_PAIR_LAST": False}, {"TEXT_MLP_PAIR_SPLIT": False}, {"TEXT_LIN_SPLIT": False},
    {"TEXT_FUSE_LN": True, "TEXT_SPLITK": True}, {"TEXT_MLP_PAIR": False, "TEXT_SPLITK": False}]
TEXT_FORMS = [("f32", False), ("f32", True), ("bf16", False), ("f16", False)]          # (operand dtype, split16_enabled())


def block_cases():
    cases = []
    for sw in BLOCK_SWITCHES:
        # (a switch setting: bf16 and fp16 take the same branches, DropPath factors and add_pos_out only change arguments)
        axes = ((1, 63, 64, 124, 125, 190, 191), ("f32", "bf16", "f16") if not sw else ("f32", "f16"), (False, True), (False, True),
                (False, True) if not sw else (True,), (True, False) if not sw else (True,), (1536, 768))
        for B, dt, save, pin, pout, dp, fc1 in itertools.product(*axes):
            cases.append(dict(B=B, dtype=dt, save=save, pos_in_x=pin, add_pos_out=pout, dp=dp, fc1=fc1, switches=sw))
    return cases


def text_cases():
    cases = []

    def add(dt, s16, eff, P, rin, layers, save, cfc, sw, C=3, Lfull=8, stage=None, gs=1.0):
        cases.append(dict(dtype=dt, split16=s16, C=C, Lfull=Lfull, eff_len=eff, prefix=P, rows_in=rin, layers=layers, save=save,
                          c_fc=cfc, grad_scale=gs, stage=stage or {}, switches=sw))
    # (layers, save, c_fc): the narrow c_fc (no text_mlp_pair) on three layers only
    depth = [(1, False, 2048), (1, True, 2048), (3, False, 2048), (3, True, 2048), (3, False, 1024), (3, True, 1024)]
    inputs = list(itertools.product((None, 6), (0, 2), (False, True)))                    # (eff_len, prefix, rows_in)
    few = [(None, 0, False), (6, 2, True)]
    for sw in TEXT_SWITCHES:
        for (dt, s16), (eff, P, rin), (layers, save, cfc) in itertools.product(TEXT_FORMS, few if sw else inputs, depth):
            add(dt, s16, eff, P, rin, layers, save, cfc, sw)
    # another precision for one half or both, the gradient scale, 4 097 rows
    for (dt, s16, other), halves in itertools.product((("bf16", False, "f32"), ("f32", True, "f16")),
                                                      (("text_attn",), ("text_mlp",), ("text_attn", "text_mlp"))):
        for (eff, P, rin), layers in itertools.product(few, (1, 3)):
            add(dt, s16, eff, P, rin, layers, True, 2048, {}, stage={h: other for h in halves})
    for (dt, s16), (eff, P, rin) in itertools.product(TEXT_FORMS, few):
        add(dt, s16, eff, P, rin, 3, True, 2048, {}, gs=1024.0)
    for (dt, s16), save, sw in itertools.product(TEXT_FORMS, (False, True), ({}, {"TEXT_FUSE_LN": True})):
        add(dt, s16, None, 0, True, 1, save, 2048, sw, C=17, Lfull=241)
        add(dt, s16, None, 0, False, 3, save, 2048, sw, C=17, Lfull=241)
    return cases


# every kernel choice the engine can make, as a pattern over launch_trace.signature(): {function: {choice: regex}}
_ATT = r"attention(_prefix)?_fwd"
COVER = {
    "vit_block": {
        "qkv: lnlin": r"^lnlin:ln attention_fwd ",
        "qkv: rowgemm with the LayerNorm prologue": r"^rowgemm:ln attention_fwd ",
        "qkv: layernorm_fwd + rowgemm": r"^layernorm_fwd rowgemm attention_fwd ",
        "qkv: layernorm_fwd + gemm": r"^layernorm_fwd gemm attention_fwd ",
        "proj: inside vit_mlp": r"attention_fwd vit_mlp:ln:proj $",
        "proj: rowgemm": r"attention_fwd rowgemm ",
        "proj: gemm": r"attention_fwd gemm ",
        "mlp: vit_mlp": r"(gemm|rowgemm) vit_mlp:ln $",
        "mlp: rowgemm + gemm": r"rowgemm:ln gemm $",
        "mlp: layernorm_fwd + gemm + gemm": r"layernorm_fwd gemm gemm $",
        "mlp: the saving form with out2": r"layernorm_fwd gemm:out2 gemm $",
    },
    "text_tower": {
        "in_proj: text_lin16": r"layernorm_fwd(_sum)? text_lin16 " + _ATT,
        "in_proj: text_lin_split": r"layernorm_fwd(_sum)? text_lin_split " + _ATT,
        "in_proj: gemm": r"layernorm_fwd(_sum)? gemm " + _ATT,
        "in_proj: rowgemm": r"rowgemm:ln " + _ATT,
        "out_proj: text_lin16": _ATT + " text_lin16 ",
        "out_proj: text_lin_split": _ATT + " text_lin_split ",
        "out_proj: gemm": _ATT + " gemm ",
        "mlp: text_mlp_pair with its LayerNorm": r"(gemm|text_lin16|text_lin_split) text_mlp_pair:ln ",
        "mlp: text_mlp_pair behind a LayerNorm launch": r"layernorm_fwd text_mlp_pair ",
        "mlp: gemm_splitk": r"layernorm_fwd gemm(:out2)? gemm_splitk4 layernorm_fwd_sum ",
        "mlp: plain gemm": r"layernorm_fwd gemm(:out2)? gemm (layernorm_fwd|rowgemm)",
        "mlp: rowgemm with the LayerNorm prologue": r"gemm rowgemm:ln(:out2)? gemm ",
        "layernorm_fwd_sum as hand-over": r"layernorm_fwd_sum (gemm|text_lin16|text_lin_split) " + _ATT,
        "layernorm_fwd_sum as the last layer's fold": r"layernorm_fwd_sum layernorm_fwd rows_matmul ",
        "backward mlp: text_mlp_pair": r"\|.* text_mlp_pair:bwd layernorm_bwd_sum ",
        "backward mlp: gemm + gemm_splitk x 4": r"\|.* gemm gemm_splitk4 layernorm_bwd_sum ",
        "backward mlp: gemm + gemm": r"\|.* gemm gemm layernorm_bwd gemm attention",
        "backward: text_lin16 on both dX products": r"\|.* text_lin16 attention(_prefix)?_bwd text_lin16 layernorm_bwd_sum ",
        "backward: text_lin_split on both dX products": r"\|.* text_lin_split attention(_prefix)?_bwd text_lin_split layernorm_bwd_sum ",
        "backward: gemm_splitk x 3": r"\|.* gemm attention(_prefix)?_bwd gemm_splitk3 layernorm_bwd_sum ",
        "backward: gemm + layernorm_bwd": r"\|.* gemm attention(_prefix)?_bwd gemm layernorm_bwd ",
        "backward: attention_bwd": r"\|.* attention_bwd ",
        "backward: attention_prefix_bwd": r"\|.* attention_prefix_bwd ",
    },
}


def record(cases_of):
    texts, index, out = [], {}, {}
    for fn, cases in cases_of.items():
        rows = []
        for case in cases:
            text = LT.TRACERS[fn](case)
            if text not in index:
                index[text] = len(texts)
                texts.append(text)
            rows.append(dict(case=case, sha1=hashlib.sha1(text.encode()).hexdigest(), trace=index[text]))
        out[fn] = rows
        used = sorted({r["trace"] for r in rows})
        sigs = [LT.signature(texts[i]) for i in used]
        for choice, pat in COVER[fn].items():
            assert any(re.search(pat, s) for s in sigs), f"{fn}: no recorded case runs '{choice}'"
        print(f"{fn}: {len(rows)} cases, {len(used)} distinct traces, {len(COVER[fn])} kernel choices covered")
    return out, texts


def main():
    cases, texts = record({"vit_block": block_cases(), "text_tower": text_cases()})
    if os.path.exists(OUT):
        with gzip.open(OUT, "rt") as f:
            old = json.load(f)
        if old["cases"] == cases and old["traces"] == texts:
            print(f"{OUT}: unchanged (recorded at {old['commit']})")
            return
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    blob = json.dumps(dict(commit=commit, cases=cases, traces=texts), sort_keys=True, separators=(",", ":")).encode()
    with open(OUT, "wb") as f, gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0, compresslevel=9) as z:
        z.write(blob)
    print(f"{OUT}: {sum(len(v) for v in cases.values())} cases, {len(texts)} distinct traces, {os.path.getsize(OUT)} bytes, commit {commit}")


if __name__ == "__main__":
    main()
