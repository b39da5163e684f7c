"""What tests/test_packed_io_api.py and tests/test_gpu_packed_io.py share: the shape grid, the weight matrices, and the
2-bit image's layout restated in numpy from the text of include/tcsc_gpu.h (never from the library's code)."""
import numpy as np

KS = (1, 15, 16, 17, 255, 256, 257, 300, 1025)  # around the 16-k dword, the 256-k block, and several blocks
NS = (1, 15, 16, 17, 33)                        # around the 16-column tile, and three tiles
FILLS = ("zero", "0.67", "plus", "minus")
SHARD = (5, 21)                                 # columns [5, 21) of N = 33: both ends inside a tile

_SHIFT = np.array([8 * (j & 3) + 2 * (j >> 2) for j in range(16)], np.uint64)


def weights(K, N, fill):
    """A K x N float32 matrix of -1, 0, +1: all zero, density 0.67 with random signs, all +1 or all -1."""
    if fill == "zero":
        return np.zeros((K, N), np.float32)
    if fill == "plus":
        return np.ones((K, N), np.float32)
    if fill == "minus":
        return -np.ones((K, N), np.float32)
    rng = np.random.default_rng(19000 + 7 * K + 11 * N)
    W = rng.choice(np.array([-1.0, 1.0], np.float32), (K, N))
    W[rng.random((K, N)) >= float(fill)] = 0.0
    return W


def layout_image(Wd):
    """The image of a dense ternary K x N matrix as uint8: tiles of 16 columns x 256 k, 1 KiB each, column-tile major
    then k block; lane l's dword i holds k = 256 kb + 64 i + 16 (l >> 4) + j of column 16 t + (l & 15); the code
    c = w + 1 sits at bit 8 (j & 3) + 2 (j >> 2); padding holds code 1.  Dwords are little-endian."""
    K, N = Wd.shape
    nt, nkb = (N + 15) // 16, (K + 255) // 256
    codes = np.ones((nkb * 256, nt * 16), np.uint64)
    codes[:K, :N] = (Wd + 1).astype(np.uint64)
    c = codes.reshape(nkb, 4, 4, 16, nt, 16)                   # [kb, i, quarter, j, t, column in tile]
    p = (c << _SHIFT[None, None, None, :, None, None]).sum(axis=3)  # [kb, i, quarter, t, column]: disjoint bits
    p = p.transpose(3, 0, 2, 4, 1)                             # [t, kb, quarter, column, i] = [t, kb, l, i]
    return np.ascontiguousarray(p).astype("<u4").reshape(-1).view(np.uint8)


def image_byte(k, col, K):
    """(byte index, bit shift) of the code of weight (k, col) in the image of a matrix of K rows."""
    nkb = (K + 255) // 256
    kk, j = k % 256, k % 16
    lane = 16 * ((kk % 64) // 16) + col % 16
    dword = (((col // 16) * nkb + k // 256) * 64 + lane) * 4 + kk // 64
    return 4 * dword + (j & 3), 2 * (j >> 2)


def poke(image, k, col, K, code):
    """A copy of the image with the code at (k, col) replaced; (k, col) may be a padding position."""
    out = image.copy()
    b, s = image_byte(k, col, K)
    out[b] = (int(out[b]) & ~(3 << s) & 0xFF) | (code << s)
    return out


# the three corruptions an image is refused for: (name, K, N, (k, col, code), a word of the message)
CORRUPTIONS = (
    ("code3", 300, 17, (7, 3, 3), "code 3"),
    ("pad_k", 300, 17, (300, 0, 2), "padding"),   # k = K
    ("pad_col", 300, 17, (0, 17, 0), "padding"),  # column = N
)
