"""SHA-256 of every output of every host reference under tests/ and oracle/ of a given tree, to hold two trees' references bit for bit:

    python scripts/measure/ref_bits_ab.py PATH/TO/TREE [--out digests.json]

Run it once per tree (a checkout of the parent commit and the new one) and compare the two files: a refactor of the tests' shared helpers must
leave them equal. CPU only. For every reference module it runs reference_and_bound and emulate (for optim_ref the replay) on the module's own
smallest listed cases, one per family and per operand combination, and hashes every array that comes back: dtype, shape and bytes. The
modules are imported from the tree given, in a child process, so that the script of one tree can measure another.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys


def leaves(prefix, obj, out):
    """flatten dicts, tuples and lists down to arrays and scalars: {path: sha256}"""
    import numpy as np
    if isinstance(obj, dict):
        for k in sorted(obj, key=str):
            leaves(f"{prefix}.{k}", obj[k], out)
    elif isinstance(obj, (tuple, list)):
        for i, v in enumerate(obj):
            leaves(f"{prefix}[{i}]", v, out)
    elif obj is None:
        out[prefix] = "None"
    else:
        a = np.ascontiguousarray(np.asarray(obj))
        out[prefix] = hashlib.sha256(f"{a.dtype} {a.shape} ".encode() + a.tobytes()).hexdigest()


def child(root):
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import numpy as np
    import attention_grad_ref as aref
    import embedding_grad_ref as eref
    import gemm_ref
    import layernorm_grad_ref as nref
    import linear_grad_ref as lref
    import mhop_loss_ref
    import optim_ref
    import overflow_ref
    from oracle import attention_oracle as ao
    from oracle import trunk_rows_oracle as tr
    out = {}

    def put(name, obj):
        leaves(name, obj, out)

    def grid(shape, seed, scale=1.0):  # inputs only, this script's own: multiples of 1/8, so that old values are exact in every format
        return (np.random.default_rng([seed, *shape]).integers(-16, 17, size=shape) / 8.0 * scale).astype(np.float32)

    def grid16(shape, seed):
        return grid(shape, seed).astype(np.float16)

    lens = [1, 33, 97, 130]  # one key; a ragged pair-tile; two ring jobs; three chunks of the backward
    for fam, make in ao.FAMILIES.items():
        qkv, cu = make(lens, 2, 3)
        for kernel in (1, 2, 3):
            put(f"attention_oracle {fam} kernel={kernel} reference_and_bound", ao.reference_and_bound(qkv, cu, 2, kernel))
            put(f"attention_oracle {fam} kernel={kernel} emulate", ao.emulate(qkv, cu, 2, kernel))
    qkv, cu, exp = ao.onehot(lens, 2, 3)
    put("attention_oracle onehot", (qkv, cu, exp, ao.emulate(qkv, cu, 2, 2)))

    for fam, (_, in_types, epss) in tr.LN_FAMILIES.items():
        for in_type in in_types:
            for residual in ("none", "res16", "res32"):
                c = tr.ln_case(fam, in_type, residual, 3, 64, 5)
                x, dx = tr.ln_inputs(c["inp"], c["res"])
                put(f"trunk_rows_oracle {fam} {in_type} {residual}", (tr.layer_norm(x, c["g"], c["b"], epss[0]), tr.bound(x, dx, c["g"], c["b"], epss[0])))

    for fam in aref.FAMILY_NAMES:
        qkv, cu = ao.FAMILIES[fam](lens, 2, 4)
        for mode in (0, 3):
            dctx = aref.dctx_grid(len(lens) if mode == 3 else int(cu[-1]), 128, 6)
            put(f"attention_grad_ref {fam} mode={mode} reference_and_bound", aref.reference_and_bound(qkv, dctx, cu, 2, mode))
            put(f"attention_grad_ref {fam} mode={mode} emulate", aref.emulate(qkv, dctx, cu, 2, mode))
            put(f"attention_grad_ref {fam} mode={mode} ds_feed", aref.ds_feed(qkv, dctx, cu, 2, mode))

    for M, N, K in ((1, 64, 64), (65, 192, 64), (129, 128, 128)):
        x, w, dy = lref.realistic(M, N, K, 7)
        pre = (x.astype(np.float64) @ w.astype(np.float64).T * 8 + lref.bias(N, 7)).astype(np.float16)
        old_dw, old_db = grid((N, K), 8).astype(np.float32), grid((N,), 9).astype(np.float32)
        for name, kw in (("plain", {}), ("gelu", dict(pre=pre)), ("gelu rows old", dict(pre=pre, m=M - 1, old_dw=old_dw, old_db=old_db))):
            put(f"linear_grad_ref M={M} N={N} K={K} {name} reference_and_bound", lref.reference_and_bound(x, w, dy, **kw))
            put(f"linear_grad_ref M={M} N={N} K={K} {name} emulate", lref.emulate(x, w, dy, **kw))
    x, w, dy = lref.subnormal_columns_case()
    put("linear_grad_ref subnormal columns", (lref.reference_and_bound(x, w, dy), lref.emulate(x, w, dy), lref.aligned_dw(x, dy)))
    every16 = np.arange(0, 65536, 7, dtype=np.uint16).view(np.float16)
    every16 = every16[np.isfinite(every16)]
    put("linear_grad_ref gelu_grad", (lref.gelu_grad32(every16), lref.gelu_grad64(every16), lref.gelu_grad_bound(every16)))

    for fam in nref.FAMILIES:
        for combo in nref.COMBOS:
            for M, H in ((5, 64), (9, 256)):
                c = nref.make_case(fam, combo, M, H, 3)
                old = dict(old_dg=grid((H,), 12, 4.0), old_db=grid((H,), 13, 4.0))
                put(f"layernorm_grad_ref {fam} {combo} M={M} H={H} reference_and_bound", nref.reference_and_bound(**c, m=M - 1, **old))
                put(f"layernorm_grad_ref {fam} {combo} M={M} H={H} emulate", nref.emulate(**c, m=M - 1, **old))

    for fam in eref.FAMILIES:
        for form in eref.DY_FORMS:
            B, L = eref.BL_SWEEP[3]
            c = eref.make_case(fam, 64, B, L, 5, form=form)
            old = {"dword": grid(c["word"].shape, 6, 4.0), "dpos": grid(c["pos"].shape, 7, 4.0), "dtype0": grid((64,), 8, 4.0),
                   "dg": grid((64,), 9, 4.0), "db": grid((64,), 10, 4.0)}
            put(f"embedding_grad_ref {fam} {form} reference_and_bound", eref.reference_and_bound(c, old=old))
            put(f"embedding_grad_ref {fam} {form} emulate", eref.emulate(c, old=old, accumulate=True))
    c = eref.make_case("unit", 64, 7, 50, 5)
    put("embedding_grad_ref plan", eref.plan(c))

    M, N, K = 65, 128, 64
    x, w, b, res = grid16((M, K), 1), grid16((N, K), 2), gemm_ref.grid_bias(N, 3), grid16((M, N), 4)
    put("gemm_ref grid exact", (gemm_ref.exact(x, w, b), gemm_ref.exact(x, w, b, res), gemm_ref.round16(gemm_ref.exact(x, w, b))))
    x, w, _ = gemm_ref.realistic(M, N, K, 5)
    b, res = gemm_ref.bias(N, 5), gemm_ref.realistic(M, N, K, 6)[2]
    for epilogue in (0, 1, 2, 3):
        r = res if epilogue == 2 else None
        put(f"gemm_ref realistic epilogue={epilogue} reference_and_bound", gemm_ref.reference_and_bound(x, w, b, epilogue, r))
        put(f"gemm_ref realistic epilogue={epilogue} emulate", gemm_ref.emulate(x, w, b, epilogue, r))
    lx, lw, lb, u = gemm_ref.ladder()
    put("gemm_ref ladder", (gemm_ref.gelu32(u), gemm_ref.gelu64(u), gemm_ref.gelu_bound(u), gemm_ref.gelu_err32(u, 1e-3)))
    for m in gemm_ref.GELU_MUTATIONS:
        put(f"gemm_ref ladder {m}", gemm_ref.gelu32(u, m))

    params, targets = optim_ref.trajectory_start()
    final, st = optim_ref.replay_trajectory(params, targets, 3)
    put("optim_ref replay_trajectory", (final, {k: np.asarray(v) for k, v in st.items()}))
    put("optim_ref constants", (optim_ref.NORM_REL_BOUND,))

    for B, d, K in ((3, 64, 0), (5, 64, 4)):
        inp, queue = mhop_loss_ref.make_inputs(B, d, K, seed=B + d + K)
        for o1 in (False, True):
            put(f"mhop_loss_ref B={B} K={K} o1={int(o1)}", mhop_loss_ref.loss_and_grads(inp, queue, g0=4.0, o1=o1))

    M, rows, N, K = overflow_ref.LINEAR_SHAPES[0]
    for gelu in (False, True):
        put(f"overflow_ref linear gelu={int(gelu)}", overflow_ref.linear_case(M, rows, N, K, gelu))
    put("overflow_ref layernorm", overflow_ref.layernorm_case(*overflow_ref.LN_SHAPES[0], "dy16+dy2"))
    for mode in (0, 3):
        put(f"overflow_ref attention mode={mode}", overflow_ref.attention_case(mode))
    put("overflow_ref loss", overflow_ref.loss_case())

    # the whole-encoder references WITHOUT dropout (their fp64 arithmetic repeats its bits; regime_b's fp32 index backward does not)
    import encoder_chain_ref as ch
    from oracle import seeded
    for gn, geom in (("TINY", seeded.TINY), ("DEEP", seeded.DEEP)):
        sd = ch.state_dict(geom)
        ids, mask = ch.batch("L48", geom)
        G = ch.cotangent(len(ids), geom)
        put(f"encoder_chain_ref {gn} L48 model64", ch.grads_cotangent("model64", sd, geom, ids, mask, G))
        for scale in (1.0, 256.0):
            put(f"encoder_chain_ref {gn} L48 regime scale={scale:g}", ch.grads_cotangent("regime", sd, geom, ids, mask, G, scale))
    for kind in ("model64", "regime"):
        put(f"encoder_chain_ref TINY loss {kind}", ch.grads_loss(kind, ch.state_dict(seeded.TINY), seeded.TINY, ch.loss_batches(seeded.TINY)))
    print(json.dumps(out, sort_keys=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("tree", help="root of the tree whose tests/ and oracle/ are measured")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    root = os.path.abspath(a.tree)
    if a.child:
        return child(root)
    if not os.path.isdir(os.path.join(root, "tests")):
        sys.exit(f"no tests/ under {root}")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), root, "--child"], capture_output=True, text=True, cwd=root)
    if p.returncode != 0:
        print(f"{root}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
        sys.exit(1)
    digests = json.loads(p.stdout.strip().split("\n")[-1])
    text = json.dumps(digests, indent=0, sort_keys=True) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(f"{len(digests)} digests, sha256 of all: {hashlib.sha256(text.encode()).hexdigest()}")


if __name__ == "__main__":
    main()
