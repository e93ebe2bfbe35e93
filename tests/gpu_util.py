"""helpers shared by the -m gpu parity tests: run the HIP path through the C ABI (via
haplohyped_varawareml_amd.device) and bring results back as numpy for comparison with the oracle."""
import numpy as np
import torch

from haplohyped_varawareml_amd import device as dev


def to_dev(buf):
    a = np.frombuffer(bytes(buf), dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf.view(np.uint8).reshape(-1)
    t = torch.empty(a.size + 16, dtype=torch.uint8, device="cuda")   # 16 B of slack keeps slicing aligned
    if a.size:
        t[:a.size] = torch.from_numpy(a.copy())
    return t[:a.size]


def gpu_encode(ctx, text, n_samples, region="", sc=dev.DEFAULT_SC, vc=dev.DEFAULT_VC, cap=None):
    """-> dict(G int8 [S, n_kept, 2], start, stop, ref, alt, stats, n_kept, res) like oracle.vcf_encode"""
    t = text if torch.is_tensor(text) else to_dev(text)
    lay = None
    if cap is not None or sc != dev.DEFAULT_SC or vc != dev.DEFAULT_VC:
        if cap is None:
            cap = t.numel() // (16 + 2 * max(n_samples, 0)) + 1
        lay = dev.make_layout(n_samples, cap, sc=sc, vc=vc)
    res = ctx.encode_text(t, n_samples, region=region, layout=lay)
    n = res.n_kept
    G = res.dense().cpu().numpy() if n_samples > 0 else np.zeros((0, n, 2), np.int8)
    return dict(G=np.ascontiguousarray(G), start=res.start[:n].cpu().numpy().view(np.uint32),
                stop=res.stop[:n].cpu().numpy().view(np.uint32), ref=res.ref[:n].cpu().numpy(),
                alt=res.alt[:n].cpu().numpy(), stats=res.stats, n_kept=n, res=res)


def assert_same_as_oracle(g, o):
    assert g["n_kept"] == o["n_kept"]
    assert np.array_equal(g["G"], o["G"]), "genotype matrix differs from the oracle"
    assert np.array_equal(g["start"], o["start"]) and np.array_equal(g["stop"], o["stop"])
    assert np.array_equal(g["ref"], o["ref"]) and np.array_equal(g["alt"], o["alt"])
    for k in ("n_records", "n_kept", "n_drop_region", "n_drop_filter", "n_haploid_padded"):
        assert g["stats"][k] == o["stats"][k], (k, g["stats"], o["stats"])


def split_chunks(dst, chunk_off, total):
    d = dst[:total].cpu().numpy()
    off = chunk_off.cpu().numpy()
    return [d[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def gpu_encode_one_pass(ctx, text, n_samples, region="", mode=2, planes=False, sc=dev.DEFAULT_SC, vc=dev.DEFAULT_VC, cap=None,
                        max_lines=None):
    """One pass of the line index `mode` (hhgt_set_index_mode) and the encoders, the way the ingest engine, the converter
    and bench.py run them: hhgt_encode_text_async, or (planes=True, vc % 4096 == 0) hhgt_encode_text_planes_async followed
    by hhgt_planes_expand.  No retry: a MALFORMED pass raises its HhgtError, where gpu_encode would scan every byte once
    more.  max_lines: the caller's bound (default: every line of the text).  -> the same dict as gpu_encode"""
    import torch
    t = text if torch.is_tensor(text) else to_dev(text)
    S = n_samples
    if cap is None:
        cap = t.numel() // (16 + 2 * max(S, 0)) + 1
    lay = dev.make_layout(S, cap, sc=sc, vc=vc)
    n_cap = lay.v_capacity
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=ctx.device)
    P = None
    if planes:
        assert dev.planes_bytes(lay) > 0, "the planes form needs vc % 4096 == 0"
        P = z(dev.planes_bytes(lay), torch.uint8)
    res = dev.EncodeResult(z(max(dev.layout_bytes(lay), 16), torch.uint8), lay, z(n_cap, torch.int32), z(n_cap, torch.int32),
                           z(n_cap, torch.uint8), z(n_cap, torch.uint8), 0, {}, [], P)
    cursor = z(1, torch.int64)
    if max_lines is None:
        max_lines = int((t == 0x0A).sum().item()) + 2      # the caller's bound: every line of the text (blank ones included)
    ctx.set_index_mode(mode)
    try:
        if planes:
            rec = ctx.encode_text_planes_async(t, S, res, cursor, max_lines=max_lines, region=region).wait()
        else:
            rec = ctx.encode_text_async(t, S, res, cursor, max_lines=max_lines, region=region).wait()
    finally:
        ctx.set_index_mode(-1)
    n = int(rec.stats.n_kept)
    assert int(cursor.item()) == n
    if planes:
        res.G = ctx.planes_expand(res)
    res.n_kept, res.stats, res.chrom_runs = n, rec.stats.asdict(), rec.chrom_runs()
    G = res.dense().cpu().numpy() if S > 0 else np.zeros((0, n, 2), np.int8)
    return dict(G=np.ascontiguousarray(G), start=res.start[:n].cpu().numpy().view(np.uint32),
                stop=res.stop[:n].cpu().numpy().view(np.uint32), ref=res.ref[:n].cpu().numpy(),
                alt=res.alt[:n].cpu().numpy(), stats=res.stats, n_kept=n, res=res)


ONE_PASS_FORMS = [(m, p) for m in (1, 2) for p in (False, True)]   # (index mode, planes form) of every one-pass leg


def assert_one_pass(ctx, text, n_samples, want, region="", flaggable=False, forms=ONE_PASS_FORMS, **kw):
    """One pass in each (mode, planes) of `forms` against the oracle's `want`.  flaggable=False: the text holds none of the
    shapes DESIGN.md lets one pass flag, so the pass must equal the oracle.  flaggable=True: equal to the oracle or
    "Error parsing VCF file", never a different matrix.  -> number of flagged passes"""
    from haplohyped_varawareml_amd._lib import HhgtError
    flagged = 0
    for mode, planes in forms:
        try:
            g = gpu_encode_one_pass(ctx, text, n_samples, region=region, mode=mode, planes=planes, **kw)
        except HhgtError as e:
            if not flaggable or "Error parsing VCF file" not in str(e):
                raise AssertionError(f"one pass (mode {mode}, planes {planes}) failed on valid text: {e}") from e
            flagged += 1
            continue
        if want is None:
            raise AssertionError(f"one pass (mode {mode}, planes {planes}) accepted text the oracle rejects")
        try:
            assert_same_as_oracle(g, want)
        except AssertionError as e:
            raise AssertionError(f"one pass (mode {mode}, planes {planes}): {e}") from e
    return flagged
