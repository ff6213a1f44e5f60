"""HBM data layouts of the decode path — pure tensor reshuffles, no arithmetic.

* weight tiles: bf16 ``[strip=n/16][ktile=k/32][lane][8]`` with lane ``l`` holding
  ``W[32*ktile + 8*(l>>4) + j][16*strip + (l&15)]`` — the B operand of ``v_mfma_f32_16x16x32_bf16``;
* activation planes: bf16 ``[3][mtile=m/16][ktile][lane][8]`` with lane ``l`` holding
  ``X[16*mtile + (l&15)][32*ktile + 8*(l>>4) + j]`` — the A operand; the three planes sum to the
  fp32 value exactly.

The reference stores DenseGeneral kernels as ``in_shapes + out_features`` (dia/layers.py:47-51); the
functions below flatten them to ``[K, N]`` first.
"""

from __future__ import annotations

from typing import Tuple

import torch


def _ceil(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def tile_weight(w2d: torch.Tensor) -> Tuple[torch.Tensor, int, int]:
    """[K, N] float -> (bf16 tiles [N/16, K/32, 64, 8], K/32, N/16); K, N zero-padded to 32 / 16."""
    K, N = w2d.shape
    Kp, Np = _ceil(K, 32), _ceil(N, 16)
    if (Kp, Np) != (K, N):
        wp = torch.zeros(Kp, Np, dtype=w2d.dtype, device=w2d.device)
        wp[:K, :N] = w2d
        w2d = wp
    kt, ns = Kp // 32, Np // 16
    t = w2d.reshape(kt, 4, 8, ns, 16).permute(3, 0, 1, 4, 2)        # (strip, kt, kq, c, j)
    return t.reshape(ns, kt, 64, 8).to(torch.bfloat16).contiguous(), kt, ns


def tile_weight_planes(w2d: torch.Tensor) -> Tuple[torch.Tensor, int, int]:
    """[K, N] fp32 -> (bf16 tiles [3, N/16, K/32, 64, 8], K/32, N/16): the hi / mid / lo planes of the weights
    (hi + mid + lo == w exactly), one tile set each, back to back — dia_gemm_args.w_planes = 3."""
    planes = [tile_weight(pl.float()) for pl in split3(w2d.float())]
    return torch.stack([t for t, _, _ in planes]).contiguous(), planes[0][1], planes[0][2]


def tile_weight_bf16x2(w2d: torch.Tensor) -> Tuple[torch.Tensor, int, int]:
    """[K, N] fp32 -> (bf16 tiles [N/16, 2*K/32, 64, 8], 2*K/32, N/16): the hi = bf16(w) and lo = bf16(w - hi) planes of the weights
    (|hi + lo - w| <= 2^-17 |w|), INTERLEAVED per k-tile inside each strip — weight k-tile j is plane j & 1 of activation k-tile
    j >> 1, so a strip stays one sequential stream and a split-K range over the doubled k-tiles holds both planes of its K
    range — dia_gemm_args.w_planes = 2."""
    hi, lo = split2(w2d.float())
    th, kt, ns = tile_weight(hi.float())
    tl, _, _ = tile_weight(lo.float())
    return torch.stack([th, tl], dim=2).reshape(ns, 2 * kt, 64, 8).contiguous(), 2 * kt, ns


def untile_weight_bf16x2(tiles: torch.Tensor, K: int, N: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """inverse of tile_weight_bf16x2: the (hi, lo) planes as fp32 [K, N] (their sum approximates w)"""
    ns, kt2 = tiles.shape[0], tiles.shape[1]
    t = tiles.reshape(ns, kt2 // 2, 2, 64, 8)
    return untile_weight(t[:, :, 0], K, N), untile_weight(t[:, :, 1], K, N)


def untile_weight(tiles: torch.Tensor, K: int, N: int) -> torch.Tensor:
    ns, kt = tiles.shape[0], tiles.shape[1]
    w = tiles.float().reshape(ns, kt, 4, 16, 8).permute(1, 2, 4, 0, 3).reshape(kt * 32, ns * 16)
    return w[:K, :N].contiguous()


def split2(x: torch.Tensor):
    """fp32 -> (hi, lo) bf16 with hi = bf16(x), lo = bf16(x - hi): 16 significand bits, relative error <= 2^-17"""
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return hi, lo


def split3(x: torch.Tensor):
    hi = x.to(torch.bfloat16)
    r = x - hi.float()
    mid = r.to(torch.bfloat16)
    lo = (r - mid.float()).to(torch.bfloat16)
    return hi, mid, lo


def pack_planes(x: torch.Tensor, ktiles: int | None = None, mtiles: int | None = None) -> torch.Tensor:
    """fp32 [M, K] -> bf16 planes [3, mtiles, ktiles, 64, 8]."""
    M, K = x.shape
    mt = mtiles if mtiles is not None else _ceil(M, 16) // 16
    kt = ktiles if ktiles is not None else _ceil(K, 32) // 32
    xp = torch.zeros(mt * 16, kt * 32, dtype=torch.float32, device=x.device)
    xp[:M, :K] = x
    out = []
    for pl in split3(xp):
        out.append(pl.reshape(mt, 16, kt, 4, 8).permute(0, 2, 3, 1, 4).reshape(mt, kt, 64, 8))
    return torch.stack(out).contiguous()


def unpack_planes(p: torch.Tensor, M: int, K: int) -> torch.Tensor:
    """inverse of pack_planes (sums the three planes in fp32)."""
    _, mt, kt = p.shape[:3]
    s = p[0].float() + p[1].float() + p[2].float()
    x = s.reshape(mt, kt, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(mt * 16, kt * 32)
    return x[:M, :K].contiguous()


def pack_f32_tiles(x: torch.Tensor, ktiles: int | None = None, mtiles: int | None = None) -> torch.Tensor:
    """fp32 [M, K] -> fp32 activation tiles [mtiles, ktiles, 64, 8]: the fragment order of one plane with 4-byte elements
    (dia_gemm_args.act_f32; the 5..128-row kernels split the planes in registers)."""
    M, K = x.shape
    mt = mtiles if mtiles is not None else _ceil(M, 16) // 16
    kt = ktiles if ktiles is not None else _ceil(K, 32) // 32
    xp = torch.zeros(mt * 16, kt * 32, dtype=torch.float32, device=x.device)
    xp[:M, :K] = x
    return xp.reshape(mt, 16, kt, 4, 8).permute(0, 2, 3, 1, 4).reshape(mt, kt, 64, 8).contiguous()


def unpack_f32_tiles(t: torch.Tensor, M: int, K: int) -> torch.Tensor:
    """inverse of pack_f32_tiles"""
    mt, kt = t.shape[:2]
    return t.reshape(mt, kt, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(mt * 16, kt * 32)[:M, :K].contiguous()


def interleave_gate_up(wi: torch.Tensor) -> torch.Tensor:
    """wi_fused kernel [D, 2, F] (layers.py:77-82) -> [D, 2F] where every 16-column strip holds
    8 gate columns followed by the 8 matching up columns."""
    D, two, F = wi.shape
    assert two == 2 and F % 8 == 0
    g = wi[:, 0, :].reshape(D, F // 8, 8)
    u = wi[:, 1, :].reshape(D, F // 8, 8)
    return torch.cat([g, u], dim=2).reshape(D, 2 * F)


def rope_pair_perm(head_dim: int = 128) -> torch.Tensor:
    """column order inside a head so that a RoPE pair (d, d+head_dim/2) sits in adjacent columns."""
    c = torch.arange(head_dim)
    return (c // 2) + (head_dim // 2) * (c % 2)


def rope_tables(npos: int, head_dim: int, min_ts: int, max_ts: int):
    """cos/sin [npos, head_dim/2] fp32 built with the reference's op sequence
    (dia/layers.py:126-132, 145-146, 161-162): inv_freq = 1/(min*(max/min)**(2i/H)), theta = pos*inv_freq."""
    half = head_dim // 2
    fraction = (2.0 * torch.arange(0, half)) / head_dim
    inv_freq = (1.0 / (min_ts * (max_ts / min_ts) ** fraction)).to(torch.float32)
    pos = torch.arange(npos, dtype=torch.float32)
    f = pos.unsqueeze(-1) * inv_freq
    return torch.cos(f.to(torch.float32)).contiguous(), torch.sin(f.to(torch.float32)).contiguous()


def v_to_blocked(v: torch.Tensor) -> torch.Tensor:
    """V cache [..., T, 128] -> blocked [..., T/32, 128, 32] (the MFMA attention kernel's B operand wants
    8 consecutive KEYS of one dim in 16 bytes); same number of elements, T % 32 == 0."""
    *lead, T, H = v.shape
    return v.reshape(*lead, T // 32, 32, H).transpose(-1, -2).contiguous()


def v_from_blocked(vb: torch.Tensor) -> torch.Tensor:
    *lead, nb, H, k = vb.shape
    return vb.transpose(-1, -2).reshape(*lead, nb * k, H).contiguous()


SPARSE_HEADER = 80          # bytes: 64 lane masks + 4 x uint16 row prefixes + 8 pad


def sparse_tile_weight(tiles: torch.Tensor):
    """bf16 weight tiles [ns, kt, 64, 8] -> (blocks uint8 [bytes], toff int32 [ns*kt]) — the zero-skipping stream
    format for unstructured-pruned matrices (offline_prune.py --prune-mode unstructured):

      block of a tile = [64 x uint8 lane masks (bit j = element j of the lane's 8-element fragment is non-zero)]
                        [4 x uint16: non-zeros in lanes < 16*q]  [8 pad bytes]
                        [non-zero bf16 values, lane-major]                 padded to 16 bytes, <= 1024 bytes
      a tile with more than 472 non-zeros is stored raw (1024 bytes, the dense fragment order)
      toff[tile] = (block offset / 16) << 8 | (block size / 16, or 0 for a raw tile)

    One 16-byte load per lane still fetches a whole tile (lanes past the block re-read its last chunk), so the
    kernel keeps the dense kernel's prefetch structure and simply moves fewer bytes."""
    ns, kt = tiles.shape[0], tiles.shape[1]
    dev = tiles.device
    raw = tiles.contiguous().view(torch.int16).reshape(ns * kt, 64, 8)
    nzm = raw != 0                                                    # [T, 64, 8]
    cnt = nzm.sum(dim=2)                                              # [T, 64]
    nnz = cnt.sum(dim=1)                                              # [T]
    dense = nnz > 472
    size = torch.where(dense, torch.full_like(nnz, 1024), (SPARSE_HEADER + 2 * nnz + 15) // 16 * 16)
    off = torch.cumsum(size, 0) - size
    total = int(size.sum().item())
    blocks = torch.zeros(total, dtype=torch.uint8, device=dev)
    T = ns * kt
    # raw tiles
    if bool(dense.any()):
        idx = torch.nonzero(dense).flatten()
        dst = (off[idx][:, None] + torch.arange(1024, device=dev)[None, :]).reshape(-1)
        blocks[dst] = raw[idx].reshape(len(idx), -1).view(torch.uint8).reshape(-1)
    sp = ~dense
    if bool(sp.any()):
        idx = torch.nonzero(sp).flatten()
        bits = (nzm[idx].to(torch.int32) * (1 << torch.arange(8, device=dev, dtype=torch.int32))[None, None, :]).sum(dim=2)   # [S, 64]
        dst = (off[idx][:, None] + torch.arange(64, device=dev)[None, :]).reshape(-1)
        blocks[dst] = bits.to(torch.uint8).reshape(-1)
        rowpre = torch.cumsum(cnt[idx].reshape(len(idx), 4, 16).sum(dim=2), dim=1) - cnt[idx].reshape(len(idx), 4, 16).sum(dim=2)   # [S, 4]
        rp = rowpre.to(torch.int16).contiguous().view(torch.uint8).reshape(len(idx), 8)
        dst = (off[idx][:, None] + 64 + torch.arange(8, device=dev)[None, :]).reshape(-1)
        blocks[dst] = rp.reshape(-1)
        # values: global order of the non-zeros is already (tile, lane, j)
        sel = nzm[idx]
        vals = raw[idx][sel]                                           # int16 [sum nnz]
        tile_of = torch.repeat_interleave(torch.arange(len(idx), device=dev), nnz[idx])
        start = torch.cumsum(nnz[idx], 0) - nnz[idx]
        within = torch.arange(vals.numel(), device=dev) - start[tile_of]
        dstb = off[idx][tile_of] + SPARSE_HEADER + 2 * within
        vb = vals.contiguous().view(torch.uint8).reshape(-1, 2)
        blocks[dstb] = vb[:, 0]
        blocks[dstb + 1] = vb[:, 1]
    chunks = torch.where(dense, torch.zeros_like(size), size // 16)
    toff = ((off // 16) << 8 | chunks).to(torch.int32)
    return blocks, toff.contiguous()


def sparse_untile(blocks: torch.Tensor, toff: torch.Tensor, ns: int, kt: int) -> torch.Tensor:
    """inverse of sparse_tile_weight (test helper, slow): bf16 tiles [ns, kt, 64, 8]"""
    b = blocks.cpu().numpy()
    t = toff.cpu().numpy().astype("int64") & 0xFFFFFFFF
    import numpy as np
    out = np.zeros((ns * kt, 64, 8), dtype=np.int16)
    for i in range(ns * kt):
        o, ch = int(t[i] >> 8) * 16, int(t[i] & 255)
        if ch == 0:
            out[i] = b[o: o + 1024].view(np.int16).reshape(64, 8)
            continue
        masks = b[o: o + 64]
        vals = b[o + SPARSE_HEADER: o + ch * 16].view(np.int16)
        k = 0
        for l in range(64):
            for j in range(8):
                if masks[l] >> j & 1:
                    out[i, l, j] = vals[k]; k += 1
    return torch.from_numpy(out).view(torch.bfloat16).reshape(ns, kt, 64, 8)


# ---- 2:4 sparse weight stream (dia_gemm_args.w_format = DIA_W_SPARSE24, csrc/gemm_sparse.hip) ---------------------------
SP24_GROUP = 8           # sparse k-tiles (64 K each) behind one metadata block


def tile_weight_24(w2d: torch.Tensor) -> Tuple[torch.Tensor, int, int]:
    """[K, N] float, at most 2 non-zeros in every group of 4 consecutive K of a column (pruning.is_2of4) -> (stream bf16
    [N/16, G, 9, 64, 8], K/64, N/16): the compressed A operand of ``v_smfmac_f32_16x16x64_bf16``.  K is zero-padded to a
    multiple of 64 (one sparse k-tile), N to 16, the k-tiles to whole groups of 8 (G = ceil(K/64 / 8)).

    Operand mapping (pinned on the hardware by tests/test_gpu_sparse24.py): lane l of sparse k-tile t holds the 8 kept values of
    output column 16 strip + (l & 15) over K = 64 t + 16 (l >> 4) + [0, 16): value j belongs to group g = j >> 1
    (K 64 t + 16 (l >> 4) + 4 g + [0, 4)); the lower kept position is j = 2g, the higher j = 2g + 1.  Its position inside the
    group (0..3) sits in bits [2j + 1 : 2j] of a 16-bit index word; the instruction's index operand carries two such words,
    selected by ``abid`` (0: bits 0-15, 1: bits 16-31).  The dense B operand (16 bf16 per lane) holds activation row l & 15 at
    K = 64 t + 32 (e >> 3) + 8 (l >> 4) + (e & 7) for element e: the two halves are exactly the A fragments of the dense
    k-tiles 2t and 2t + 1 (fp32 activation tiles, pack_f32_tiles).

    Stream of a strip: one block per group of 8 sparse k-tiles, each a sequential 9 KiB = slot 0, the metadata (16 bytes per lane:
    dword d = index words of k-tiles 2d (bits 0-15) and 2d + 1 (bits 16-31) of the group), then slots 1..8, the values of the
    group's k-tiles (16 bytes per lane).  A group with fewer than 2 non-zeros in a K group of 4 keeps zero-valued positions
    (lowest first), so every index word names two distinct positions in increasing order.  0.5625 of the dense tiles' bytes."""
    K, N = w2d.shape
    Kp, Np = _ceil(K, 64), _ceil(N, 16)
    kt, ns = Kp // 64, Np // 16
    G = (kt + SP24_GROUP - 1) // SP24_GROUP
    wp = torch.zeros(G * SP24_GROUP * 64, Np, dtype=torch.float32, device=w2d.device)
    wp[:K, :N] = w2d.float()
    g = wp.reshape(-1, 4, Np)                                                  # [K/4, 4, N]
    nz = (g != 0).to(torch.int32)
    if bool((nz.sum(dim=1) > 2).any()):
        raise ValueError("tile_weight_24: more than 2 non-zeros in a group of 4 consecutive K (prune with pruning.semi_structured_prune_state_dict)")
    # non-zeros first, then the lowest positions; the two picks in increasing position order
    key = (1 - nz) * 4 + torch.arange(4, device=w2d.device).view(1, 4, 1)
    pos = torch.sort(torch.topk(key, 2, dim=1, largest=False).indices, dim=1).values       # [K/4, 2, N]
    val = torch.gather(g, 1, pos)
    kt8 = G * SP24_GROUP
    # (t, q, g, s, strip, c) -> (strip, t, lane = 16 q + c, j = 2 g + s)
    val = val.reshape(kt8, 4, 4, 2, ns, 16).permute(4, 0, 1, 5, 2, 3).reshape(ns, kt8, 64, 8)
    pos = pos.reshape(kt8, 4, 4, 2, ns, 16).permute(4, 0, 1, 5, 2, 3).reshape(ns, kt8, 64, 8)
    word = (pos.to(torch.int64) << (2 * torch.arange(8, device=w2d.device, dtype=torch.int64))).sum(dim=3)  # [ns, kt8, 64]
    word = word.reshape(ns, G, 4, 2, 64)
    dword = word[:, :, :, 0] | (word[:, :, :, 1] << 16)                                       # [ns, G, 4, 64]
    meta = dword.permute(0, 1, 3, 2).to(torch.int32).contiguous().view(torch.int16)           # [ns, G, 64, 8] int16
    vals = val.to(torch.bfloat16).reshape(ns, G, SP24_GROUP, 64, 8)
    stream = torch.cat([meta.view(torch.bfloat16).reshape(ns, G, 1, 64, 8), vals], dim=2)
    return stream.contiguous(), kt, ns


def untile_weight_24(stream: torch.Tensor, K: int, N: int) -> torch.Tensor:
    """inverse of tile_weight_24 (test helper): fp32 [K, N]"""
    ns, G = stream.shape[0], stream.shape[1]
    kt8 = G * SP24_GROUP
    meta = stream[:, :, 0].contiguous().view(torch.int16).reshape(ns, G, 64, 8).view(torch.int32).to(torch.int64) & 0xFFFFFFFF  # [ns, G, 64, 4]
    word = torch.stack([meta & 0xFFFF, meta >> 16], dim=-1).permute(0, 1, 3, 4, 2).reshape(ns, kt8, 64)                    # [ns, kt8, 64]
    pos = (word[..., None] >> (2 * torch.arange(8, dtype=torch.int64, device=stream.device))) & 3                           # [ns, kt8, 64, 8]
    val = stream[:, :, 1:].float().reshape(ns, kt8, 64, 8)
    # (strip, t, q, c, g, s) -> dense [t, q, g, 4 positions, strip, c]
    val = val.reshape(ns, kt8, 4, 16, 4, 2).permute(1, 2, 4, 5, 0, 3)
    pos = pos.reshape(ns, kt8, 4, 16, 4, 2).permute(1, 2, 4, 5, 0, 3)
    dense = torch.zeros(kt8, 4, 4, 4, ns, 16, dtype=torch.float32, device=stream.device)
    dense.scatter_add_(3, pos[:, :, :, 0:1], val[:, :, :, 0:1])
    dense.scatter_add_(3, pos[:, :, :, 1:2], val[:, :, :, 1:2])
    return dense.reshape(kt8 * 64, ns * 16)[:K, :N].contiguous()


# ---- MXFP8 weight stream (dia_gemm_args.w_format = DIA_W_MXFP8, csrc/gemm_mx.hip) ------------------------------------
FP8_GROUP = 16                           # k-tiles (32 K each) behind one scale block
FP8_GROUP_BYTES = 256 + 8 * 1024         # scale block + 8 value slots


def tile_weight_fp8(w2d: torch.Tensor) -> Tuple[torch.Tensor, int, int]:
    """[K, N] float -> (stream uint8 [N/16, G, 8448], K/32, N/16): the MXFP8 encoding of the matrix (quant.mxfp8_quantize_2d: e4m3
    elements, one E8M0 scale per 32 consecutive K of a column = per column of a k-tile) in the order csrc/gemm_mx.hip reads.
    K is zero-padded to a multiple of 32, N to 16, the k-tiles to whole groups of 16 (G = ceil(K/32 / 16)).

    Stream of a strip: one block per group of 16 k-tiles, each a sequential 8448 bytes = a 256-byte scale block
    ``[16 columns][16 k-tiles]`` (lane l of a wave reads the bytes of column l & 15), then 8 slots of 1 KiB: slot p =
    ``[64 lanes][16 bytes]``, lane l holding its 8 elements of k-tile 2p (bytes 0-7) and of k-tile 2p + 1 (bytes 8-15), element
    j of k-tile t = W[32 t + 8 (l >> 4) + j][16 strip + (l & 15)] as in the dense tiles.  0.515625 of the dense tiles' bytes."""
    from .quant import mxfp8_quantize_2d
    K, N = w2d.shape
    Np = _ceil(N, 16)
    kt, ns = _ceil(K, 32) // 32, Np // 16
    G = (kt + FP8_GROUP - 1) // FP8_GROUP
    el, sc = mxfp8_quantize_2d(w2d)
    elp = torch.zeros(G * FP8_GROUP * 32, Np, dtype=torch.uint8, device=w2d.device)
    scp = torch.full((G * FP8_GROUP, Np), 127, dtype=torch.uint8, device=w2d.device)
    elp[: el.shape[0], :N] = el
    scp[: sc.shape[0], :N] = sc
    # (G, p, h, kq, j, strip, c) -> (strip, G, p, lane = 16 kq + c, byte = 8 h + j)
    vals = elp.reshape(G, 8, 2, 4, 8, ns, 16).permute(5, 0, 1, 3, 6, 2, 4).reshape(ns, G, 8 * 1024)
    scales = scp.reshape(G, FP8_GROUP, ns, 16).permute(2, 0, 3, 1).reshape(ns, G, 256)
    return torch.cat([scales, vals], dim=2).contiguous(), kt, ns


def untile_weight_fp8(stream: torch.Tensor, K: int, N: int) -> torch.Tensor:
    """inverse of tile_weight_fp8 (test helper): the DEQUANTISED matrix, fp32 [K, N]"""
    from .quant import mxfp8_dequantize_2d
    ns, G = stream.shape[0], stream.shape[1]
    scales = stream[:, :, :256].reshape(ns, G, 16, FP8_GROUP).permute(1, 3, 0, 2).reshape(G * FP8_GROUP, ns * 16)
    vals = stream[:, :, 256:].reshape(ns, G, 8, 4, 16, 2, 8).permute(1, 2, 5, 3, 6, 0, 4).reshape(G * FP8_GROUP * 32, ns * 16)
    return mxfp8_dequantize_2d(vals.contiguous(), scales.contiguous())[:K, :N].contiguous()


# ---- MXFP4 weight stream (dia_gemm_args.w_format = DIA_W_MXFP4, csrc/gemm_mx.hip) ------------------------------------
FP4_GROUP_BYTES = 256 + 4 * 1024         # scale block + 4 value slots (FP8_GROUP k-tiles)


def tile_weight_fp4(w2d: torch.Tensor) -> Tuple[torch.Tensor, int, int]:
    """[K, N] float -> (stream uint8 [N/16, G, 4352], K/32, N/16): the MXFP4 encoding of the matrix (quant.mxfp4_quantize_2d: e2m1
    elements, one E8M0 scale per 32 consecutive K of a column) in the order csrc/gemm_mx.hip reads.  K is zero-padded to a
    multiple of 32, N to 16, the k-tiles to whole groups of 16 (G = ceil(K/32 / 16)).

    Stream of a strip: one block per group of 16 k-tiles, each a sequential 4352 bytes = the 256-byte scale block of
    tile_weight_fp8 (``[16 columns][16 k-tiles]``), then 4 slots of 1 KiB: slot p = ``[64 lanes][16 bytes]``, lane l holding its
    8 elements of k-tile 4p + i in bytes 4i .. 4i + 3 (one dword per k-tile), element j of k-tile t =
    W[32 t + 8 (l >> 4) + j][16 strip + (l & 15)] as in the dense tiles.  Element j sits in byte j >> 1 of the dword, the even
    element in the LOW nibble: v_cvt_scalef32_pk_bf16_fp4 with byte select b returns (low nibble, high nibble) of byte b as the
    (first, second) bf16 of its result, so selects 0..3 give elements 0..7 in order (pinned on the hardware by
    tests/test_gpu_mxfp4.py::test_operand_probe).  0.265625 of the dense tiles' bytes."""
    from .quant import mxfp4_quantize_2d
    K, N = w2d.shape
    Np = _ceil(N, 16)
    kt, ns = _ceil(K, 32) // 32, Np // 16
    G = (kt + FP8_GROUP - 1) // FP8_GROUP
    el, sc = mxfp4_quantize_2d(w2d)
    elp = torch.zeros(G * FP8_GROUP * 32, Np, dtype=torch.uint8, device=w2d.device)
    scp = torch.full((G * FP8_GROUP, Np), 127, dtype=torch.uint8, device=w2d.device)
    elp[: el.shape[0], :N] = el
    scp[: sc.shape[0], :N] = sc
    # (G, p, i, kq, byte, nibble, strip, c) -> (strip, G, p, lane = 16 kq + c, 4 i + byte)
    nib = elp.reshape(G, 4, 4, 4, 4, 2, ns, 16)
    vals = (nib[:, :, :, :, :, 0] | (nib[:, :, :, :, :, 1] << 4)).permute(5, 0, 1, 3, 6, 2, 4).reshape(ns, G, 4 * 1024)
    scales = scp.reshape(G, FP8_GROUP, ns, 16).permute(2, 0, 3, 1).reshape(ns, G, 256)
    return torch.cat([scales, vals], dim=2).contiguous(), kt, ns


def untile_weight_fp4(stream: torch.Tensor, K: int, N: int) -> torch.Tensor:
    """inverse of tile_weight_fp4 (test helper): the DEQUANTISED matrix, fp32 [K, N]"""
    from .quant import mxfp4_dequantize_2d
    ns, G = stream.shape[0], stream.shape[1]
    scales = stream[:, :, :256].reshape(ns, G, 16, FP8_GROUP).permute(1, 3, 0, 2).reshape(G * FP8_GROUP, ns * 16)
    by = stream[:, :, 256:].reshape(ns, G, 4, 4, 16, 4, 4)                    # (strip, G, p, kq, c, i, byte)
    nib = torch.stack([by & 15, by >> 4], dim=-1)                            # ... nibble
    codes = nib.permute(1, 2, 5, 3, 6, 7, 0, 4).reshape(G * FP8_GROUP * 32, ns * 16)
    return mxfp4_dequantize_2d(codes.contiguous(), scales.contiguous())[:K, :N].contiguous()


# ---- unstructured sparse weight stream (dia_gemm_args.w_format = DIA_W_USPARSE, csrc/gemm_us.hip) ---------------------
US_GROUP = 16                            # k-tiles (32 K each) behind one mask block
US_RATES = (4, 2)                        # bf16 slots of a lane's window per k-tile


def us_group_bytes(rate: int) -> int:
    """mask block + value slots of one group: 9 KiB at rate 4, 5 KiB at rate 2 (16 KiB dense)"""
    return 1024 + rate * 2048


def us_stream_bytes(nstrips: int, groups: int, rate: int, n_overflow: int) -> int:
    """bytes of the stream tile_weight_us returns: fixed part + run table + overflow entries (each padded to 16) + 16"""
    return (nstrips * groups * us_group_bytes(rate) + _ceil(4 * (nstrips * groups * 16 + 1), 16)
            + _ceil(4 * n_overflow, 16) + 16)


def _us_lane_tiles(w2d: torch.Tensor):
    """[K, N] -> int16 bf16 bits [ns, G, 16 k-tiles, 64 lanes, 8] in the dense B-operand mapping, K padded to whole groups"""
    K, N = w2d.shape
    Np = _ceil(N, 16)
    kt, ns = _ceil(K, 32) // 32, Np // 16
    G = (kt + US_GROUP - 1) // US_GROUP
    wp = torch.zeros(G * US_GROUP * 32, Np, dtype=torch.bfloat16, device=w2d.device)
    wp[:K, :N] = w2d.to(torch.bfloat16)
    # (G, i, kq, j, strip, c) -> (strip, G, i, lane = 16 kq + c, j)
    t = wp.reshape(G, US_GROUP, 4, 8, ns, 16).permute(4, 0, 1, 2, 5, 3).reshape(ns, G, US_GROUP, 64, 8).contiguous()
    return t, kt, ns, G


def tile_weight_us(w2d: torch.Tensor, rate: int) -> Tuple[torch.Tensor, int, int]:
    """[K, N] float -> (stream uint8 [bytes], K/32, N/16): the bf16 values of an unstructured-pruned matrix as a lane-local
    fixed-rate stream plus an overflow list, in the order csrc/gemm_us.hip reads.  Lossless for any matrix (a dense one spills
    everything beyond `rate` per lane and k-tile).  K is zero-padded to a multiple of 32, N to 16, the k-tiles to whole groups
    of 16 (G = ceil(K/32 / 16)).  "Non-zero" is ``value != 0`` after rounding to bf16: a negative zero is dropped.

    Lane l of k-tile t of a strip owns the dense B-operand elements j = 0..7 = W[32 t + 8 (l >> 4) + j][16 strip + (l & 15)].
    The stream is three parts back to back:

    1. fixed part ``[ns][G][us_group_bytes(rate)]``.  A group of 16 k-tiles is a 1 KiB mask block ``[64 lanes][16 bytes]``
       (byte i of lane l = the mask of k-tile i of the group, bit j = element j is non-zero) followed by value slots of 1 KiB
       ``[64 lanes][16 bytes]``.  A lane's WINDOW of a k-tile is its first `rate` non-zeros in element order as bf16, the rest
       of the window zero.  rate 4: slot p holds the windows (8 bytes) of k-tiles 2p, 2p + 1 — 8 slots, 9 KiB per group;
       rate 2: slot p holds the windows (4 bytes) of k-tiles 4p .. 4p + 3 — 4 slots, 5 KiB per group.
    2. run table, uint32 ``[ns * G * 16 + 1]`` at byte ns * G * us_group_bytes(rate): entry (strip * G + g) * 16 + c is the index
       of the first overflow entry of column c of group g of the strip; the last entry is the total.  Padded to 16 bytes.
    3. overflow entries, uint32 each, ordered by (strip, group, column, k): ``k within the group (0..511) | bf16 bits << 16``,
       the non-zeros of a lane and k-tile beyond its window.  Padded to 16 bytes, then 16 zero bytes.

    us_stream_bytes(ns, G, rate, entries) is the size.  Every read of the kernel (clamped prefetches included) lies inside.
    The returned K/32 is ceil(K / 32) as for the other tilers, while the stream holds G * 16 k-tiles per strip: dia_gemm takes
    KT = G * 16 only, i.e. the two agree for K a multiple of 512 and a stream of any other K is for untile_weight_us alone."""
    if rate not in US_RATES:
        raise ValueError("tile_weight_us: rate must be 4 or 2")
    t, kt, ns, G = _us_lane_tiles(w2d)
    dev = t.device
    bits = t.view(torch.int16)
    nz = t != 0                                                         # (-0.0 != 0 is false: dropped)
    nzi = nz.to(torch.int64)
    rank = torch.cumsum(nzi, dim=-1) - nzi                              # non-zeros before element j
    mask = (nzi << torch.arange(8, device=dev)).sum(dim=-1)             # [ns, G, 16, 64]
    keep, spill = nz & (rank < rate), nz & (rank >= rate)
    win = torch.zeros(ns, G, US_GROUP, 64, rate + 1, dtype=torch.int16, device=dev)
    win.scatter_(-1, torch.where(keep, rank, torch.full_like(rank, rate)), torch.where(keep, bits, torch.zeros_like(bits)))
    slot_kt = 8 // rate                                                 # k-tiles per value slot
    vals = win[..., :rate].reshape(ns, G, US_GROUP // slot_kt, slot_kt, 64, rate).permute(0, 1, 2, 4, 3, 5)
    vals = vals.contiguous().view(torch.uint8).reshape(ns, G, -1)
    masks = mask.permute(0, 1, 3, 2).to(torch.uint8).reshape(ns, G, 1024)
    fixed = torch.cat([masks, vals], dim=2).reshape(-1)
    # overflow: (strip, G, i, kq, c, j) -> (strip, G, c, i, kq, j), so that nonzero() walks the runs in (column, k) order
    sp = spill.reshape(ns, G, US_GROUP, 4, 16, 8).permute(0, 1, 4, 2, 3, 5)
    sb = bits.reshape(ns, G, US_GROUP, 4, 16, 8).permute(0, 1, 4, 2, 3, 5)
    idx = torch.nonzero(sp)                                             # [E, 6]
    kk = 32 * idx[:, 3] + 8 * idx[:, 4] + idx[:, 5]
    ent = kk | ((sb[sp].to(torch.int64) & 0xFFFF) << 16)
    cnt = sp.reshape(ns * G * 16, -1).sum(dim=1)
    table = torch.zeros(ns * G * 16 + 1, dtype=torch.int64, device=dev)
    table[1:] = torch.cumsum(cnt, 0)

    def u32_bytes(v, pad):
        b = (v.to(torch.int64)[:, None] >> (8 * torch.arange(4, device=dev))) & 0xFF
        out = torch.zeros(_ceil(4 * v.numel(), 16) + pad, dtype=torch.uint8, device=dev)
        out[: 4 * v.numel()] = b.to(torch.uint8).reshape(-1)
        return out
    stream = torch.cat([fixed, u32_bytes(table, 0), u32_bytes(ent, 16)]).contiguous()
    assert stream.numel() == us_stream_bytes(ns, G, rate, int(ent.numel()))
    return stream, kt, ns


def untile_weight_us(stream: torch.Tensor, K: int, N: int, rate: int) -> torch.Tensor:
    """inverse of tile_weight_us (test helper): fp32 [K, N]"""
    kt, ns = _ceil(K, 32) // 32, _ceil(N, 16) // 16
    G = (kt + US_GROUP - 1) // US_GROUP
    dev = stream.device
    gb = us_group_bytes(rate)
    fixed = stream[: ns * G * gb].reshape(ns, G, gb)
    mask = fixed[:, :, :1024].reshape(ns, G, 64, US_GROUP).permute(0, 1, 3, 2).to(torch.int64)            # [ns, G, 16, 64]
    slot_kt = 8 // rate
    win = fixed[:, :, 1024:].contiguous().view(torch.int16).reshape(ns, G, US_GROUP // slot_kt, 64, slot_kt, rate)
    win = win.permute(0, 1, 2, 4, 3, 5).reshape(ns, G, US_GROUP, 64, rate)
    nz = (mask[..., None] >> torch.arange(8, device=dev)) & 1
    rank = torch.cumsum(nz, dim=-1) - nz
    keep = (nz == 1) & (rank < rate)
    bits = torch.where(keep, torch.gather(win, -1, rank.clamp(max=rate - 1)), torch.zeros((), dtype=torch.int16, device=dev))
    nt = ns * G * 16 + 1
    to = ns * G * gb

    def u32(b):
        return (b.reshape(-1, 4).to(torch.int64) << (8 * torch.arange(4, device=dev))).sum(dim=1)
    table = u32(stream[to: to + 4 * nt])
    eo = to + _ceil(4 * nt, 16)
    ent = u32(stream[eo: eo + 4 * int(table[-1])])
    run = torch.repeat_interleave(torch.arange(nt - 1, device=dev), table[1:] - table[:-1])
    strip, g, c = run // (G * 16), (run // 16) % G, run % 16
    kk = ent & 0x1FF
    v = ((ent >> 16) - ((ent >> 31) << 16)).to(torch.int16)
    bits = bits.contiguous()
    bits[strip, g, kk >> 5, 16 * ((kk >> 3) & 3) + c, kk & 7] = v
    return untile_weight(bits.view(torch.bfloat16).reshape(ns, G * US_GROUP, 64, 8), K, N)


def us_choose(w2d: torch.Tensor, max_ratio: float = 1.0):
    """the smaller of the two streams of a matrix, or None when it is not below max_ratio of the dense tiles' bytes:
    (stream, rate, K/32, N/16, stream bytes, dense bytes).  K/32 and N/16 are tile_weight_us's: ceil(K / 32), NOT padded to the
    whole groups the stream holds — the kernel takes KT a multiple of 16 only, so K must be a multiple of 512 for a stream that
    is to be launched (DeviceWeights checks it); the dense bytes count the same unpadded k-tiles"""
    best = None
    for rate in US_RATES:
        s, kt, ns = tile_weight_us(w2d, rate)
        if best is None or s.numel() < best[0].numel():
            best = (s, rate, kt, ns)
    s, rate, kt, ns = best
    dense = ns * kt * 1024
    if s.numel() >= max_ratio * dense:
        return None
    return s, rate, kt, ns, int(s.numel()), dense


# ---- ring layout of the persistent MLP segment (csrc/seg.hip) ------------------------------------------------------
SEG_CUS = 256            # one workgroup per CU of an MI355X
SEG_K = 2048             # contraction length of one slot (16 tiles of 128 k x 4 columns)


def _seg_slots(w2d: torch.Tensor) -> torch.Tensor:
    """[2048, N] float (N % 4 == 0) -> bf16 [N/4, 16, 64, 8]: one 16 KiB slot per group of 4 columns.  Tile t, lane l,
    element j = W[128 t + 32 ((l & 15) >> 2) + 8 (l >> 4) + j][4 group + (l & 3)] — four k-tiles of the four columns side
    by side in the 16 B-operand columns of v_mfma_f32_16x16x32_bf16 (the matching A operand carries the rows of k-tile g in
    rows 4g..4g+3, so the product is block diagonal)."""
    K, N = w2d.shape
    if K != SEG_K or N % 4:
        raise ValueError("seg slots: K must be 2048 and N a multiple of 4")
    lane = torch.arange(64, device=w2d.device)
    t = torch.arange(16, device=w2d.device)
    j = torch.arange(8, device=w2d.device)
    k = (128 * t[:, None, None] + (32 * ((lane & 15) >> 2) + 8 * (lane >> 4))[None, :, None] + j[None, None, :])   # [16, 64, 8]
    c = (lane & 3)[None, :, None].expand(16, 64, 8)
    g = w2d.reshape(K, N // 4, 4)
    out = g[k[None], torch.arange(N // 4, device=w2d.device)[:, None, None, None], c[None]]     # [N/4, 16, 64, 8]
    return out.to(torch.bfloat16).contiguous()


def seg_ring(co: torch.Tensor, wi_gate: torch.Tensor, wi_up: torch.Tensor, wo: torch.Tensor, qkv_next) -> torch.Tensor:
    """The weights one persistent segment streams, per CU in consumption order: bf16 [256][slots][16][64][8].
      co       [2048, 2048]  cross-attention o_proj ([heads*128, D]): CU c owns columns [8c, 8c+8)           -> 2 slots
      wi_gate / wi_up [2048, 8192]: CU c owns hidden units [32c, 32c+32), gate slots then up slots          -> 16 slots
      wo       [8192, 2048]: CU c owns K quarter c >> 6 of columns [32 (c & 63), +32)                        -> 8 slots
      qkv_next [2048, 3072] or None (last layer): CU c owns columns [12c, 12c+12)                            -> 3 slots"""
    D, F = co.shape[1], wi_gate.shape[1]
    if co.shape != (SEG_K, 2048) or wi_gate.shape != (2048, 8192) or wi_up.shape != (2048, 8192) or wo.shape != (8192, 2048):
        raise ValueError("seg_ring: built for the Dia-1.6B decoder shapes")
    parts = [_seg_slots(co).reshape(SEG_CUS, 2, 16, 64, 8),
             _seg_slots(wi_gate).reshape(SEG_CUS, 8, 16, 64, 8), _seg_slots(wi_up).reshape(SEG_CUS, 8, 16, 64, 8)]
    # wo: [quarter q][K 2048][2048 columns] -> slots [q][512 groups] -> CU (q, c) takes groups [8c, 8c+8)
    wo_s = torch.stack([_seg_slots(wo[q * SEG_K:(q + 1) * SEG_K]) for q in range(4)])            # [4, 512, 16, 64, 8]
    parts.append(wo_s.reshape(4, 64, 8, 16, 64, 8).reshape(SEG_CUS, 8, 16, 64, 8))
    if qkv_next is not None:
        if qkv_next.shape != (2048, 3072):
            raise ValueError("seg_ring: q/k/v projection must be [2048, 3072]")
        parts.append(_seg_slots(qkv_next).reshape(SEG_CUS, 3, 16, 64, 8))
    return torch.cat(parts, dim=1).contiguous()


def diag_tile_weight(w2d: torch.Tensor) -> torch.Tensor:
    """[K, N] float (K % 128 == 0, N % 4 == 0) -> bf16 [N/4, K/128, 64, 8]: the diagonal layout of dia_gemm_args.w_layout = 1 (k_gemv_diag).
    Tile t of column group g, lane l, element j = W[128 t + 32 ((l & 15) >> 2) + 8 (l >> 4) + j][4 g + (l & 3)]: four k-tiles of the group's
    four columns side by side in the B operand of v_mfma_f32_16x16x32_bf16 (as the slots of seg_ring, for any K)."""
    K, N = w2d.shape
    if K % 128 or N % 4:
        raise ValueError("diag_tile_weight: K must be a multiple of 128 and N of 4")
    lane = torch.arange(64, device=w2d.device)
    t = torch.arange(K // 128, device=w2d.device)
    j = torch.arange(8, device=w2d.device)
    k = (128 * t[:, None, None] + (32 * ((lane & 15) >> 2) + 8 * (lane >> 4))[None, :, None] + j[None, None, :])      # [K/128, 64, 8]
    c = (lane & 3)[None, :, None].expand(K // 128, 64, 8)
    g = w2d.reshape(K, N // 4, 4)
    out = g[k[None], torch.arange(N // 4, device=w2d.device)[:, None, None, None], c[None]]
    return out.to(torch.bfloat16).contiguous()
