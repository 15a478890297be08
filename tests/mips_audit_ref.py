"""Helper of tests/test_mips_audit_*.py: the report of emdr2_mips_audit restated on the host.

`sound_reference`: numpy float64 from the raw buffers of a shard copied to the host -- words 0-4, 7-9 and 12 (12 over the sound words and
the padding words only).  The layout is restated here from DESIGN section 4, not read back through `unpack_rows`: block (t, c) of the fp16
image -- stripe t = rows [128 t, 128 t + 128), chunk c = elements [32 c, 32 c + 32) -- is 8 KiB at ((t * nch) + c) * 8192 and holds 512
slots of 16 bytes, the 8-element group s of row r at slot r * 4 + (s ^ ((r >> 2) & 3)); the int8 image has the same geometry with half
the chunks (64 elements per chunk, 16 per slot).

`canonical_reference` (needs the GPU): words 5, 6, 10, 11, 13 and the rows behind word 10, by running the project's own
`emdr2_mips_block_norms` / `emdr2_mips_seal_shadow` into scratch buffers and comparing bytes on the host.

`full_reference` puts the two together: all 14 named words."""
import ctypes

import numpy as np

NONE = (1 << 64) - 1


def _logical(image_bytes, elems_per_slot, dtype, dim):
    """stripe-tiled bytes -> [padded rows, dim] in logical order."""
    per_chunk = elems_per_slot * 4
    nch = dim // per_chunk
    a = np.frombuffer(np.ascontiguousarray(image_bytes).tobytes(), dtype=dtype).reshape(-1, nch, 128, 4, elems_per_slot)   # [t, c, r, slot, e]
    r = np.arange(128)
    slot = np.arange(4)[None, :] ^ ((r >> 2) & 3)[:, None]                          # [r, s] -> slot of group s
    a = np.take_along_axis(a, slot[None, None, :, :, None], axis=3)                  # [t, c, r, s, e]
    return a.transpose(0, 2, 1, 3, 4).reshape(-1, dim)


def tiled_rows_bits(tiled, dim):
    """fp16 image bytes -> uint16 [padded rows, dim]"""
    return _logical(tiled, 8, np.uint16, dim)


def shadow_rows(image, dim):
    """int8 image bytes -> int8 [padded rows, dim]"""
    return _logical(image, 16, np.int8, dim)


def sound_reference(tiled, n_rows, dim, row_base, emax_sq, block_norm_sq=None, shadow=None, table=None):
    """-> {word index: value} for words 0-4, 7-9, and 12 over those."""
    bits = tiled_rows_bits(tiled, dim)
    padded = bits.shape[0]
    assert padded == (n_rows + 511) // 512 * 512 or (n_rows == 0 and padded == 512)
    w = {i: 0 for i in (0, 1, 2, 3, 4, 7, 8, 9)}
    w[0] = n_rows
    bad = np.zeros(padded, dtype=bool)
    if n_rows == 0:
        w[12] = NONE
        return w
    real = np.arange(padded) < n_rows
    pad_nonzero = ~real & (bits != 0).any(axis=1)
    w[1] = int(pad_nonzero.sum())
    bad |= pad_nonzero
    nonfinite = real & ((bits & 0x7c00) == 0x7c00).any(axis=1)
    w[2] = int(nonfinite.sum())
    bad |= nonfinite
    ok = real & ~nonfinite
    with np.errstate(all="ignore"):
        x = bits.view(np.float16).astype(np.float64)
        n2 = (x * x).sum(axis=1)
        norm = np.sqrt(n2)
        bound = np.float64(np.sqrt(np.float32(emax_sq)) * np.float32(1.001))        # formed in float, as the search's proof forms it
        over = ok & (norm > bound)
        w[3] = int(over.sum())
        bad |= over
        blk = np.arange(padded) >> 8
        if block_norm_sq is not None:
            low = ok & (n2 > np.asarray(block_norm_sq, dtype=np.float32).astype(np.float64)[blk] * (1.001 * 1.001))
            w[4] = int(low.sum())
            bad |= low
        if shadow is not None:
            sealed = (n_rows + 255) // 256
            in_sealed = np.arange(padded) < sealed * 256
            e8 = shadow_rows(shadow, dim)
            t = np.asarray(table, dtype=np.float32).reshape(-1, 4).astype(np.float64)
            b = np.minimum(blk, sealed - 1)
            spad = ~real & in_sealed & (e8 != 0).any(axis=1)
            w[7] = int(spad.sum())
            bad |= spad
            nlow = ok & (norm > t[b, 1])
            w[8] = int(nlow.sum())
            bad |= nlow
            r = x - t[b, 0][:, None] * e8.astype(np.float64)
            dlow = ok & (np.sqrt((r * r).sum(axis=1)) > t[b, 2])
            w[9] = int(dlow.sum())
            bad |= dlow
    w[12] = row_base + int(np.nonzero(bad)[0][0]) if bad.any() else NONE
    return w


def canonical_reference(lib, shard):
    """The canonical words of `shard` (a HipIndexShard on the GPU) by a fresh run of the project's routines into scratch buffers.
    -> ({5, 6, 10, 11, 13: value}, local rows counted in word 10)."""
    import torch
    from emdr2_amd import _native
    w = {5: 0, 6: 0, 10: 0, 11: 0, 13: NONE}
    if shard.n_rows == 0:
        return w, np.zeros(0, dtype=np.int64)
    nb = ctypes.c_size_t()
    assert lib.emdr2_mips_block_norm_bytes(shard.n_rows, ctypes.byref(nb)) == 0
    fresh = torch.empty(nb.value // 4, dtype=torch.float32, device=shard.device)
    assert lib.emdr2_mips_block_norms(shard.tiled.data_ptr(), shard.n_rows, shard.dim, 0, fresh.numel(), fresh.data_ptr(), _native.stream_ptr()) == 0
    fresh = fresh.cpu().numpy()
    bad_blocks = np.zeros(fresh.shape[0], dtype=bool)
    if shard._block_norms is not None:
        diff = fresh.view(np.uint32) != shard._block_norms.cpu().numpy().view(np.uint32)
        w[5] = int(diff.sum())
        bad_blocks |= diff
    w[6] = int(np.float32(fresh.max()).view(np.uint32) != shard.emax_sq.cpu().numpy().view(np.uint32)[0])
    rows10 = np.zeros(0, dtype=np.int64)
    if shard._shadow is not None:
        image = torch.zeros_like(shard._shadow[0])
        table = torch.zeros_like(shard._shadow[1])
        flag = torch.zeros(1, dtype=torch.int32, device=shard.device)
        assert lib.emdr2_mips_seal_shadow(shard.tiled.data_ptr(), shard.n_rows, shard.dim, image.data_ptr(), table.data_ptr(), flag.data_ptr(),
                                          _native.stream_ptr()) == 0
        sealed = (shard.n_rows + 255) // 256
        a = shadow_rows(image.cpu().numpy(), shard.dim)[:sealed * 256]
        b = shadow_rows(shard._shadow[0].cpu().numpy(), shard.dim)[:sealed * 256]
        rows10 = np.nonzero((a != b).any(axis=1))[0]
        w[10] = int(rows10.size)
        ta = table.cpu().numpy().view(np.uint32).reshape(-1, 4)[:sealed, :3]
        tb = shard._shadow[1].cpu().numpy().view(np.uint32).reshape(-1, 4)[:sealed, :3]
        diff = (ta != tb).any(axis=1)
        w[11] = int(diff.sum())
        bad_blocks[:sealed] |= diff
    if bad_blocks.any():
        w[13] = int(np.nonzero(bad_blocks)[0][0])
    return w, rows10


def full_reference(lib, shard):
    """All 14 named report words of `shard` as a list."""
    table = shard._block_norms
    sh = shard._shadow
    s = sound_reference(shard.tiled.cpu().numpy(), shard.n_rows, shard.dim, shard.row_base, float(shard.emax_sq.cpu().numpy()[0]),
                        None if table is None else table.cpu().numpy(), None if sh is None else sh[0].cpu().numpy(),
                        None if sh is None else sh[1].cpu().numpy())
    c, rows10 = canonical_reference(lib, shard)
    words = [0] * 14
    for k, v in list(s.items()) + list(c.items()):
        words[k] = v
    if rows10.size:
        words[12] = min(words[12], shard.row_base + int(rows10[0]))
    return words
