"""ddq_replay_set_augment (include/ddq_hip.h) restated: shift stream and edge-padded crop."""
import numpy as np

M64 = (1 << 64) - 1
SALT = 0xD1B54A32D192ED03


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def shift(seed, ctr, j, z, pad):
    """(dy, dx) of draw ctr's sample j, side z (0 state, 1 next_state)."""
    r = splitmix64((seed ^ SALT) ^ splitmix64((ctr * 0x100000001B3 + (2 * j + z) * 0x9E37) & M64))
    return r % (2 * pad + 1) - pad, (r >> 32) % (2 * pad + 1) - pad


def shifts(seed, ctr, B, pad):
    """The draw's blob "aug_shift": (B, 4) float32 (dy_s, dx_s, dy_s', dx_s')."""
    return np.float32([shift(seed, ctr, j, 0, pad) + shift(seed, ctr, j, 1, pad) for j in range(B)])


def shifted(frames, dy, dx):   # (..., S, S): edge-padded by 8, cropped back at (dy, dx)
    S = frames.shape[-1]
    wide = np.pad(frames, [(0, 0)] * (frames.ndim - 2) + [(8, 8), (8, 8)], mode="edge")
    return wide[..., 8 + dy:8 + dy + S, 8 + dx:8 + dx + S]


def augmented(state, nxt, sh):   # (B, 4, S, S) frames under the (B, 4) shifts
    sh = np.asarray(sh).astype(int)
    return (np.stack([shifted(f, d[0], d[1]) for f, d in zip(state, sh)]),
            np.stack([shifted(f, d[2], d[3]) for f, d in zip(nxt, sh)]))


def pattern_ring(cap, S):
    """arange-patterned frames: neighbouring pixels, rows, channels and slots all differ."""
    p = np.arange(S * S).reshape(S, S)
    s, c = np.arange(cap)[:, None, None, None], np.arange(4)[None, :, None, None]
    return ((7 * p + 29 * s + 61 * c) % 256).astype(np.uint8)
