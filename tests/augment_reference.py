"""Host replica of the augmentation of hriemo_gather_rows_aug (hri-emo_amd/csrc/store.hip, data.StoreAugment), built on the replica
of the counter hash (tests/hashrng.py): which utterances a draw drops, which rows its spans mask, the integer noise variate of
every element, and ``apply`` -- the augmented batch itself, bit for bit what the kernel writes.  Nothing here imports the package."""
import numpy as np
import torch

from hashrng import M32, fmix32, mix24, site_key, thr16

AUG_SITE = 0x41554700
CA, CB = np.uint64(0x9E3779B1), np.uint64(0x85EBCA77)
NOISE_VAR = 21845.0


def _mul(a, b):
    return (np.asarray(a, dtype=np.uint64) * b) & M32


def utterance_keys(seed, draw, modality, ids):
    """ku of every store id (uint64 array holding 32-bit values)"""
    return fmix32((site_key(seed, AUG_SITE + modality, draw) + _mul(ids, CA)) & M32)


def drop_flags(seed, draw, ids, thr_lo, thr_hi):
    """True where the utterance's rows of the launch with thresholds [thr_lo, thr_hi) are dropped (one draw for both modalities)"""
    r = fmix32((site_key(seed, AUG_SITE, draw) + _mul(ids, CA)) & M32) & np.uint64(0xFFFF)
    return (r >= np.uint64(thr_lo)) & (r < np.uint64(thr_hi))


def spans(seed, draw, modality, ids, lengths, n_spans, max_width, frac16):
    """-> (s, w), int64 [len(ids), n_spans]: span j of utterance i masks its rows s[i, j] .. s[i, j] + w[i, j]"""
    ku = utterance_keys(seed, draw, modality, ids)[:, None]
    L = np.asarray(lengths, dtype=np.uint64)[:, None]
    j = np.arange(1, n_spans + 1, dtype=np.uint64)[None, :]
    h = fmix32((ku + _mul(j, CB)) & M32)
    W = np.minimum(np.uint64(max_width), (L * np.uint64(frac16)) >> np.uint64(16))
    w = ((h & np.uint64(0xFFFF)) * (W + np.uint64(1))) >> np.uint64(16)
    s = ((h >> np.uint64(16)) * (L - w + np.uint64(1))) >> np.uint64(16)
    return s.astype(np.int64), w.astype(np.int64)


def noise_key(ku):
    return fmix32((np.asarray(ku, dtype=np.uint64) + np.uint64(0x27D4EB2F)) & M32)


def noise_k(kn, rows, cols):
    """int64 [rows, cols]: the sum of the four bytes of mix24(kn + r * CA + c * CB), minus 510"""
    r = np.arange(rows, dtype=np.uint64)[:, None]
    c = np.arange(cols, dtype=np.uint64)[None, :]
    h = mix24((np.uint64(int(kn)) + _mul(r, CA) + _mul(c, CB)) & M32)
    b = np.uint64(255)
    k = (h & b) + ((h >> np.uint64(8)) & b) + ((h >> np.uint64(16)) & b) + (h >> np.uint64(24))
    return k.astype(np.int64) - 510


def launch_cfg(which, time_mask=None, sigma=0.0, drop=(0.0, 0.0)):
    """the scalars of one launch as data.StoreAugment forms them: which = 0 audio, 1 text; time_mask = (spans, max_width, max_frac)"""
    thr_a, thr_t = thr16(drop[0]), thr16(drop[1])
    lo, hi = ((0, thr_a), (thr_a, thr_a + thr_t))[which]
    n_spans, width, frac = time_mask if time_mask is not None else (0, 0, 0.0)
    return dict(modality=which + 1, thr_lo=lo, thr_hi=hi, spans=n_spans, max_width=width, frac16=min(65536, int(frac * 65536.0 + 0.5)),
                noise_scale=float(np.float32(sigma / np.sqrt(NOISE_VAR))))


def row_masks(ids, offsets, cfg, seed, draw):
    """per batch position: bool [L] -- True where the row becomes zero (span or drop) --, and whether the utterance is dropped"""
    lengths = [offsets[i + 1] - offsets[i] for i in ids]
    dropped = drop_flags(seed, draw, ids, cfg["thr_lo"], cfg["thr_hi"])
    s, w = spans(seed, draw, cfg["modality"], ids, lengths, cfg["spans"], cfg["max_width"], cfg["frac16"])
    out = []
    for i, L in enumerate(lengths):
        m = np.zeros(L, dtype=bool)
        if dropped[i]:
            m[:] = True
        else:
            for j in range(cfg["spans"]):
                m[s[i, j]:s[i, j] + w[i, j]] = True
        out.append(m)
    return out, dropped


def apply(rows, ids, offsets, modality, cfg, seed, draw):
    """rows: the STORE's rows, a CPU tensor [N, d] (fp32, bf16 or fp16); offsets: the host offsets -> the augmented batch of `ids`
    [sum of lengths, d] in the store's dtype.  Noise: x + float32(scale) * float32(k) in numpy.float32, each operation rounded,
    cast back with torch's round-to-nearest-even; then the zeros.  With noise_scale == 0 kept rows are the store's bits."""
    assert cfg["modality"] == modality
    masks, _ = row_masks(ids, offsets, cfg, seed, draw)
    ku = utterance_keys(seed, draw, modality, ids)
    scale = np.float32(cfg["noise_scale"])
    out = []
    for i, u in enumerate(ids):
        x = rows[offsets[u]:offsets[u + 1]].clone()
        if cfg["noise_scale"] != 0.0:
            k = noise_k(noise_key(ku[i]), x.shape[0], x.shape[1]).astype(np.float32)
            y = x.float().numpy() + scale * k
            assert y.dtype == np.float32
            x = torch.from_numpy(y).to(rows.dtype)
        x[torch.from_numpy(masks[i])] = 0
        out.append(x)
    return torch.cat(out, dim=0)
