"""The device side that tests/test_encoder_chain_gpu.py, tests/test_encoder_chain_dropout_gpu.py and tests/test_overflow_chain_gpu.py share: the retriever encoder as ONE chain of the
package's differentiable functions (Chain, with a tape of every call and a hook on every output), its leaves (params), the NaN seeding of the
caching allocator (poison), the bit comparisons, and criterion E's assertion (check_e). The host side is tests/encoder_chain_ref.py.
Chain, params, poison and check_e take the geometry (oracle.seeded.TINY or DEEP); the default is TINY."""
import functools

import numpy as np
import torch

import encoder_chain_ref as ch
from multihop_dense_retrieval_amd._lib import ptr

GEOM = ch.GEOM
E_ = "encoder.embeddings."


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _ibits(t):
    t = t.detach().contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(_ibits(a), _ibits(b)))


def params(geom=GEOM):
    sd = ch.state_dict(geom)
    return {k: torch.from_numpy(v).cuda().requires_grad_(True) for k, v in sd.items()}


def poison(mib=64, geom=GEOM):
    """allocate, fill with NaN bit patterns and free blocks of the sizes the chain's torch.empty calls ask for (and many more): the caching
    allocator hands them out again, so a read of an unwritten row shows as a NaN. Then every block the allocator still holds free -- what
    earlier tests freed, the splinters between live tensors, the rest of the segments opened here -- is asked for by its exact size and
    filled too, so that no unseeded block is left for the allocator to prefer, however much ran before. The first lot is FREED before that
    second step: a request above 1 MiB that meets a free block up to 1 MiB larger is handed the whole block unsplit, and the fill writes only
    what was asked for -- held, such a block hides its unwritten rest; freed, it is one of the blocks asked for by their exact size.
    Nothing here can fault."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()  # whole free segments go back to the driver: what remains free lies inside segments with live tensors
    held, total = [], 0
    H, F = geom["hidden"], geom["ffn"]
    rows = (1280, 640, 288, 192, 8, 6, 4)
    shapes = [(r, c) for r in rows for c in (H, 3 * H, F)] + [(H, H), (3 * H, H), (F, H), (H, F), (geom["vocab"], H), (geom["max_pos"], H), (H,), (3 * H,), (F,)]
    while total < mib << 20:
        for s in shapes:  # the bytes of an fp16 and of an fp32 tensor of this shape, all ones: a NaN whichever of the two types reads them
            for width in (2, 4):  # (an fp32 NaN written as such reads as one NaN and one zero in fp16, and sizes do coincide: [1280, H] fp16, [640, H] fp32)
                held.append(torch.full((width * int(np.prod(s)),), 0xFF, dtype=torch.uint8, device="cuda"))
            total += 6 * int(np.prod(s))
        for n in (512, 4096, 65536, 1 << 20, 4 << 20):
            held.append(torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda"))
            total += n
    torch.cuda.synchronize()
    held = []
    for _ in range(8):  # a block of a small segment above 1 MiB takes two requests, a new segment's rest another pass
        free = sorted((b["size"], seg["segment_type"]) for seg in torch.cuda.memory_snapshot() for b in seg["blocks"] if b["state"] == "inactive")
        if not free:
            break
        for size, pool in reversed(free):  # (requests of up to 1 MiB are served from the small segments, larger ones from the large)
            held.append(torch.full((min(size, 1 << 20) if pool == "small" else size,), 0xFF, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    del held


class Chain:
    """one encode through the public functions, with a tape of every call and hooks on every output. half: None, or a function from a weight
    leaf to the fp16 copy that every Linear is handed as weight16 (optim.FusedAdam.half). geom: the geometry P was made for.
    dropout: None (the graph is the one without any dropout call), or (p, seed, encode): the reference's training dropout, every call at the
    site ch.site_of(encode, layer, place) -- packed_dropout(y32, ..., rows=total, also16=True) behind the embedding (the embedding's own fp16
    copy then has no consumer), dropout=(p, seed, site) on both attention forms, packed_dropout on a Linear's output in front of both
    residual LayerNorms (rows = None in the CLS tail: the mask's row index is the sequence index). Each call is on the tape as kind "drop"
    (a call whose threshold is 0 hands its input back and is not taped: there is nothing between the two stages). With a threshold of 0 the
    embedding's call is NOT made and the embedding's own fp16 copy is used: that copy is the kernel's single rounding of the unrounded value,
    fp16(y32) is a second rounding of the fp32 one, and the two differ by an fp16 ulp where y32 sits exactly between two fp16 values (a
    handful of elements per batch; tests/test_encoder_chain_dropout_gpu.py holds both facts)."""

    def __init__(self, P, ids, mask, half=None, geom=GEOM, dropout=None):
        from multihop_dense_retrieval_amd import _lib
        from multihop_dense_retrieval_amd import dropout as _dropout
        from multihop_dense_retrieval_amd.attention import packed_self_attention
        from multihop_dense_retrieval_amd.embedding import packed_embedding_layer_norm
        from multihop_dense_retrieval_amd.layernorm import packed_layer_norm
        from multihop_dense_retrieval_amd.linear import packed_linear
        self.tape, self.P, self.geom, self.dropout = [], P, geom, dropout
        NH, EPS, PAD = geom["heads"], geom["ln_eps"], geom["pad_id"]
        self.ids_np, self.mask_np = ids, mask
        B, L = ids.shape
        self.B, self.L, self.cap = B, L, B * L
        tids, tmask = torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda()
        i32 = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")  # noqa: E731
        lens, cu, total, order, src, pid = i32(B), i32(B + 1), i32(1), i32(B), i32(self.cap), i32(self.cap)
        _lib.check(_lib.lib().mdr_test_pack(ptr(tids), ptr(tmask), B, L, PAD, ptr(lens), ptr(cu), ptr(total), ptr(order), ptr(src), ptr(pid), 0, _lib.current_stream_ptr()))
        self.ids, self.cu, self.total, self.src, self.pid = tids, cu, total, src, pid
        self.T = int(mask.sum())
        self.starts = torch.from_numpy(np.concatenate([[0], np.cumsum(mask.sum(1))[:-1]]).astype(np.int64)).cuda()

        def linear(x, names, gelu=False, rows=None, label=""):
            w = P[names[0] + ".weight"] if len(names) == 1 else torch.cat([P[n + ".weight"] for n in names])
            b = P[names[0] + ".bias"] if len(names) == 1 else torch.cat([P[n + ".bias"] for n in names])
            if half is None:
                y = packed_linear(x, w, b, gelu, rows)
            else:
                w16 = half(P[names[0] + ".weight"]) if len(names) == 1 else torch.cat([half(P[n + ".weight"]) for n in names])
                y = packed_linear(x, w, b, gelu, rows, w16)
            self._rec("linear", label, {"x": x}, {"y": y}, w=w, b=b, gelu=gelu, rows=rows, names=names)
            return y

        def ln(x, res, name, rows=None, label=""):
            y16, y32 = packed_layer_norm(x, res, P[name + ".weight"], P[name + ".bias"], EPS, rows, True)
            self._rec("ln", label, {"x": x, "res": res}, {"y16": y16, "y32": y32}, rows=rows, name_=name)
            return y16, y32

        def attn(qkv, cls_only, label, i):
            if dropout is None:
                ctx = packed_self_attention(qkv, cu, NH, L, cls_only)
                self._rec("attn", label, {"qkv": qkv}, {"ctx": ctx}, mode=3 if cls_only else 0)
                return ctx
            p_, seed, enc = dropout
            site = ch.site_of(enc, i, "attn")
            ctx = packed_self_attention(qkv, cu, NH, L, cls_only, dropout=(p_, seed, site))
            T = _dropout.threshold(p_)
            self._rec("attn", label, {"qkv": qkv}, {"ctx": ctx}, mode=3 if cls_only else 0, drop=(T, seed, site) if T else None)
            return ctx

        def drop(x, i, place, rows, label, also16=False):
            """x, or with also16 (y32, y16), through the hidden dropout of site_of(encode, i, place)"""
            if dropout is None:
                return x
            p_, seed, enc = dropout
            site = ch.site_of(enc, i, place)
            y = _dropout.packed_dropout(x, p_, seed, site, rows, also16)
            if y is not x:
                self._rec("drop", label, {"x": x}, {"y32": y[0], "y16": y[1]} if also16 else {"y": y}, rows=rows, drop=(_dropout.threshold(p_), seed, site))
            return y

        def tail(p, ctx, res32, rows, lab, i):
            ao = drop(linear(ctx, [p + "attention.output.dense"], False, rows, lab + ".ao"), i, "ao", rows, lab + ".ao.drop")
            a16, a32 = ln(ao, res32, p + "attention.output.LayerNorm", rows, lab + ".ln1")
            f2 = linear(linear(a16, [p + "intermediate.dense"], True, rows, lab + ".ff1"), [p + "output.dense"], False, rows, lab + ".ff2")
            return ln(drop(f2, i, "ff2", rows, lab + ".ff2.drop"), a32, p + "output.LayerNorm", rows, lab + ".ln2")

        h16, h32 = packed_embedding_layer_norm(tids, src, pid, total, P[E_ + "word_embeddings.weight"], P[E_ + "position_embeddings.weight"],
                                               P[E_ + "token_type_embeddings.weight"][0], P[E_ + "LayerNorm.weight"], P[E_ + "LayerNorm.bias"], EPS,
                                               self.cap, PAD, True)
        self._rec("emb", "emb", {}, {"y16": h16, "y32": h32})
        if dropout is not None and _dropout.threshold(dropout[0]):
            h32, h16 = drop(h32, 0, "emb", total, "emb.drop", also16=True)
        nl = geom["layers"]
        for i in range(nl):
            p, lab = f"encoder.encoder.layer.{i}.", f"L{i}"
            qkv = linear(h16, [p + "attention.self." + n for n in ("query", "key", "value")], False, total, lab + ".qkv")
            if i < nl - 1:
                h16, h32 = tail(p, attn(qkv, False, lab + ".attn", i), h32, total, lab, i)
            else:  # the CLS rows alone; their fp16 copy (h16[starts]) has no consumer in this mode
                cls32 = h32[self.starts]
                self._rec("gather", lab + ".cls", {"src32": h32}, {"cls32": cls32})
                h16, h32 = tail(p, attn(qkv, True, lab + ".attn", i), cls32, None, lab, i)
        y = linear(h16, ["project.0"], False, None, "project.0")
        out16, out = packed_layer_norm(y, None, P["project.1.weight"], P["project.1.bias"], EPS, None, True)
        self._rec("ln", "project.1", {"x": y, "res": None}, {"y16": out16, "y32": out}, rows=None, name_="project.1")
        self.out = out

    def _rec(self, kind, label, ins, outs, **extra):
        rec = dict(kind=kind, label=label, ins=ins, outs=outs, g={}, **extra)
        for k, t in outs.items():
            if t is not None and t.requires_grad:
                t.register_hook(functools.partial(self._store, rec, k))
        self.tape.append(rec)

    @staticmethod
    def _store(rec, key, g):
        if g is not None:  # (an unused output of a two-output function: autograd passes None, nothing is materialised)
            rec["g"][key] = g.detach().clone()


def grads_np(P, scale=1.0):
    return {k: v.grad.detach().cpu().numpy().astype(np.float64) / scale for k, v in P.items()}


def check_e(g_dev, g_reg, g64, batches, title, geom=GEOM):
    rows, e_pool = ch.criterion_e(g_dev, g_reg, g64, geom)
    print(ch.table(rows, e_pool, "E " + title))
    print(f"E {title}: worst share of the bar {max(r[4] for r in rows):.3f}, worst e_dev / e_reg "
          f"{max(r[1] / r[2] for r in rows if r[2] > 0):.3f}")
    zr = ch.zero_rows(batches, geom)
    w = E_ + "word_embeddings.weight"
    assert zr.any() and not g_dev[w][zr].any() and not g64[w][zr].any(), "a word row that owns no token (or padding_idx's) has a gradient"
    assert len(ch.zero_grad_names(geom)) == geom["layers"]
    for k in ch.zero_grad_names(geom):
        print(f"E {title}: {k} max |g_dev| {np.abs(g_dev[k]).max():.3e} (mathematically zero; the query bias's {np.abs(g_dev[k.replace('key', 'query')]).max():.3e})")
    assert not ch.failures(rows), [(r[0], round(r[4], 3)) for r in ch.failures(rows)]
