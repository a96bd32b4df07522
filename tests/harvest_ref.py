"""Plain numpy restatement of csrc/k_harvest.hip: loops over frames and regions, the thinning hash in Python integers, the
augmentation by numpy.rot90 and slicing.  Test infrastructure: nothing here is shared with the code under test."""
import numpy as np

REGION_START = [0, 2, 4, 6, 8, 10, 12, 14, 16, 17]
PATCH_ORIGIN = [0, 40, 80, 120, 160, 200, 240, 280, 320, 340]
M32 = 0xffffffff


def mix32(h):
    h &= M32
    h ^= h >> 16
    h = (h * 0x85ebca6b) & M32
    h ^= h >> 13
    h = (h * 0xc2b2ae35) & M32
    h ^= h >> 16
    return h


def mix(seed, frame, q):
    h = mix32((seed & M32) ^ 0x9e3779b9)
    h = mix32(h + (frame & M32) * 0x9e3779b1)
    return mix32(h + q * 0x7f4a7c15)


def region_label(position, ri, cj):
    r0, c0 = REGION_START[ri], REGION_START[cj]
    block = np.asarray(position).reshape(19, 19)[r0:r0 + 2, c0:c0 + 2]
    return int(block[0, 0]) + 3 * int(block[0, 1]) + 9 * int(block[1, 0]) + 27 * int(block[1, 1])


def harvest_ref(goban, fgcount, state_of, positions, calm_max=16, empty_keep=256, seed=0, first_frame=0, cap=None):
    """-> (x (k, 40, 40, 3), labels (k,), src (k, 2), n_found); k = min(n_found, cap)"""
    goban, fgcount = np.asarray(goban), np.asarray(fgcount).reshape(len(goban), 19, 19)
    positions = np.asarray(positions).reshape(-1, 19, 19)
    xs, labels, src = [], [], []
    for i in range(len(goban)):
        s = int(state_of[i])
        if s < 0:
            continue
        for ri in range(10):
            for cj in range(10):
                q = 10 * ri + cj
                r0, c0 = REGION_START[ri], REGION_START[cj]
                if int(fgcount[i, r0:r0 + 2, c0:c0 + 2].sum()) > calm_max:
                    continue
                label = region_label(positions[s], ri, cj)
                if label == 0 and not (mix(seed, first_frame + i, q) & 255) < empty_keep:
                    continue
                a, b = PATCH_ORIGIN[ri], PATCH_ORIGIN[cj]
                xs.append(goban[i, a:a + 40, b:b + 40])
                labels.append(label)
                src.append((i, q))
    found = len(xs)
    k = found if cap is None else min(found, cap)
    x = np.stack(xs[:k]) if k else np.zeros((0, 40, 40, 3), np.uint8)
    return x, np.array(labels[:k], np.uint8), np.array(src[:k], np.int32).reshape(-1, 2), found


def augment_ref(x, t):
    out = np.empty_like(x)
    for k in range(len(x)):
        turned = np.rot90(x[k], int(t[k]) & 3, axes=(0, 1))
        out[k] = turned[:, ::-1] if int(t[k]) & 4 else turned
    return out


def hashed_bytes(shape, salt=0):
    """bytes that are a hash of their own index: any addressing slip shows"""
    idx = np.arange(int(np.prod(shape)), dtype=np.uint64) + np.uint64((salt * 0x9e3779b97f4a7c15) & 0xffffffffffffffff)
    idx ^= idx >> np.uint64(33)
    idx *= np.uint64(0xff51afd7ed558ccd)
    idx ^= idx >> np.uint64(29)
    return (idx & np.uint64(255)).astype(np.uint8).reshape(shape)
