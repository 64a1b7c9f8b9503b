"""The judge of the batch library (include/pikazoo_batch.h): the header's definition in numpy integers -- the Philox round keys,
the Feistel permutation with its cycle walk, and copy / gather on byte arrays -- so that every comparison is bit for bit.  Also
the generator of the column cases and the shape list of tests/test_gpu_batch.py, and the mutants that
tests/test_batch_host.py shows those cases to catch.

A COLUMN CASE is a dict of plain numbers (row_bytes, elem_bytes, the three pitches, the offsets of the two bases inside their
allocations); `make_source` fills an allocation for it with bytes that differ from row to row, `gather_bytes` / `copy_bytes`
say what the destination rows must hold.
"""
import numpy as np

from oracle.pz_oracle import philox4x32_10_numpy

KEY_XOR = (0x53485546, 0x42415443)
MUTANTS = ("no_cycle_walk", "halves_swapped_back", "five_rounds", "key_words_swapped", "row_and_step_exchanged", "tail_wrapped")
BIJECTION_M = (1, 2, 3, 5, 64, 65, 1000, 2048, 4097, (1 << 21) + 7)


def philox_key(seed, mutant=None):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = ((seed & 0xFFFFFFFF) ^ KEY_XOR[0], (seed >> 32) ^ KEY_XOR[1])
    return key[::-1] if mutant == "key_words_swapped" else key


def round_keys(seed, epoch, mutant=None):
    """K[0..5]: the first six words of the Philox blocks at counters (E_lo, E_hi, 0, 0) and (E_lo, E_hi, 1, 0)"""
    e = int(epoch)
    w = philox4x32_10_numpy((np.full(2, e & 0xFFFFFFFF), np.full(2, e >> 32), np.arange(2), np.zeros(2)), philox_key(seed, mutant))
    return [int(w[i][0]) for i in range(4)] + [int(w[0][1]), int(w[1][1])]


def half_bits(M):
    return (max(2, (int(M) - 1).bit_length()) + 1) // 2


def _mix(v):
    m32 = np.uint64(0xFFFFFFFF)
    v = (v * np.uint64(0x9E3779B1)) & m32
    v ^= v >> np.uint64(15)
    v = (v * np.uint64(0x85EBCA77)) & m32
    v ^= v >> np.uint64(13)
    v = (v * np.uint64(0xC2B2AE3D)) & m32
    v ^= v >> np.uint64(16)
    return v


def perm(p, M, seed, epoch, mutant=None, walks=None):
    """perm_E of the positions `p` (any integer array), as int64.  `walks`, a list, receives the number of passes per
    position."""
    M = int(M)
    hb = np.uint64(half_bits(M))
    mask = np.uint64((1 << int(hb)) - 1)
    K = [np.uint64(k) for k in round_keys(seed, epoch, mutant)]
    x = np.asarray(p, dtype=np.uint64).copy()
    live = np.ones(x.shape, dtype=bool)
    passes = np.zeros(x.shape, dtype=np.int64)
    while live.any():
        L, R = x[live] >> hb, x[live] & mask
        for r in range(5 if mutant == "five_rounds" else 6):
            L, R = R, L ^ (_mix(R ^ K[r]) >> (np.uint64(32) - hb))
        if mutant == "halves_swapped_back":
            L, R = R, L
        x[live] = (L << hb) | R
        passes[live] += 1
        if mutant == "no_cycle_walk":
            break
        live = x >= np.uint64(M)
    if walks is not None:
        walks.append(passes)
    return x.astype(np.int64)


def perm_scalar(p, M, seed, epoch):
    """the same in pure Python integers, one position at a time, with a Philox of its own"""
    seed &= 0xFFFFFFFFFFFFFFFF
    key = ((seed & 0xFFFFFFFF) ^ 0x53485546, (seed >> 32) ^ 0x42415443)

    def philox(c):
        k0, k1 = key
        c = list(c)
        for _ in range(10):
            p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
            c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xFFFFFFFF]
            k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
        return c

    K = (philox([epoch & 0xFFFFFFFF, epoch >> 32, 0, 0]) + philox([epoch & 0xFFFFFFFF, epoch >> 32, 1, 0]))[:6]

    def mix(v):
        v = (v * 0x9E3779B1) & 0xFFFFFFFF
        v ^= v >> 15
        v = (v * 0x85EBCA77) & 0xFFFFFFFF
        v ^= v >> 13
        v = (v * 0xC2B2AE3D) & 0xFFFFFFFF
        return v ^ (v >> 16)

    b = max(2, (M - 1).bit_length())
    hb = (b + 1) // 2
    x = p
    while True:
        L, R = x >> hb, x & ((1 << hb) - 1)
        for r in range(6):
            L, R = R, L ^ (mix(R ^ K[r]) >> (32 - hb))
        x = (L << hb) | R
        if x < M:
            return x


def minibatch_rows(M, minibatches, seed, C, mutant=None):
    """the flat source row of every output row j < B of the call with counter C"""
    M, minibatches, C = int(M), int(minibatches), int(C)
    B = M // minibatches
    E, m = divmod(C, minibatches)
    if mutant == "tail_wrapped":
        wide = -(-M // minibatches)
        p = (m * wide + np.arange(B, dtype=np.int64)) % M
    else:
        p = m * B + np.arange(B, dtype=np.int64)
    return perm(p, M, seed, E, mutant)


def source_offsets(r, n, step_pitch, game_pitch, mutant=None):
    """byte offset of flat row r from the column's base"""
    r = np.asarray(r, dtype=np.int64)
    t, g = (r % n, r // n) if mutant == "row_and_step_exchanged" else (r // n, r % n)
    return t * int(step_pitch) + g * int(game_pitch)


# ---- columns -------------------------------------------------------------------------------------------------------------------
def column(row_bytes, elem_bytes, game_extra=0, step_extra=0, dst_extra=0, src_offset=0, dst_offset=0, game_pitch=None):
    """a column case; the pitches follow from k and n in `sized`"""
    return dict(row_bytes=row_bytes, elem_bytes=elem_bytes, game_extra=game_extra, step_extra=step_extra, dst_extra=dst_extra,
                src_offset=src_offset, dst_offset=dst_offset, game_pitch=game_pitch)


def sized(case, k, n):
    """the case with its pitches for a [k, n] rollout: game rows row_bytes + game_extra apart (or `game_pitch`: a stride), steps
    n game pitches + step_extra apart"""
    c = dict(case)
    c["game_pitch"] = case["game_pitch"] if case["game_pitch"] is not None else case["row_bytes"] + case["game_extra"]
    c["step_pitch"] = max(n * c["game_pitch"], c["row_bytes"]) + case["step_extra"]
    c["dst_pitch"] = case["row_bytes"] + case["dst_extra"]
    c["M"] = k * n
    c["src_bytes"] = c["src_offset"] + (k - 1) * c["step_pitch"] + (n - 1) * c["game_pitch"] + c["row_bytes"] if n else c["src_offset"]
    return c


# every kind of row in one call: flags, 2, 4, 8 bytes, the 16-bit observation row (70 bytes, 2-byte aligned), the head (76), the
# float32 observation row (140), 288 and 512; the value column of an [n, 19] float32 head (a 4-byte row every 76 bytes); pitches
# above the row on both sides; bases at mixed offsets from 256 bytes
VARIETY = [
    column(1, 1, src_offset=3, dst_offset=5),
    column(2, 2, src_offset=2, dst_offset=6),
    column(4, 4, src_offset=4, dst_offset=12),
    column(8, 8, src_offset=8, dst_offset=24),
    column(70, 2, src_offset=2, dst_offset=14),
    column(76, 4, src_offset=0, dst_offset=4),
    column(140, 4, src_offset=12, dst_offset=8),
    column(288, 8, src_offset=16, dst_offset=0),
    column(512, 4, src_offset=0, dst_offset=16),
    column(4, 4, game_pitch=76, src_offset=72),                         # head[:, 18]
    column(140, 4, game_extra=20, step_extra=64, dst_extra=4),          # pitches above the row
    column(70, 2, game_extra=2, step_extra=6, dst_extra=58, dst_offset=2),
    column(1, 1, game_extra=2, step_extra=1, dst_extra=3, src_offset=1),
    column(8, 4, game_extra=4, step_extra=4, dst_extra=4, src_offset=4, dst_offset=4),   # 8-byte rows, 4-byte aligned
    column(512, 8, step_extra=8, dst_extra=8, src_offset=8),
    column(2, 1, src_offset=1, dst_offset=1),                           # 2-byte rows, 1-byte aligned
]
assert len(VARIETY) == 16
SIMPLE = [column(4, 4), column(140, 4), column(70, 2), column(1, 1)]


def make_source(c, seed):
    """the source allocation of a sized case: random bytes, so that rows differ and NaN payloads occur in every float width"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=c["src_bytes"], dtype=np.uint8)
    if c["row_bytes"] >= 4 and c["src_bytes"] >= c["src_offset"] + 4:
        a[c["src_offset"]:c["src_offset"] + 4] = np.frombuffer(np.uint32(0x7FC12345).tobytes(), dtype=np.uint8)  # a NaN with a payload
    return a


def read_rows(source, c, offsets):
    """[len(offsets), row_bytes]: the rows at `offsets` from the column's base"""
    at = c["src_offset"] + np.asarray(offsets, dtype=np.int64)[:, None] + np.arange(c["row_bytes"], dtype=np.int64)[None, :]
    return source[at]


def gather_bytes(source, c, n, rows):
    """what the destination rows of a gather hold; a row outside [0, k * n) is zeros"""
    rows = np.asarray(rows, dtype=np.int64)
    M = c["M"]
    ok = (rows >= 0) & (rows < M)
    out = np.zeros((len(rows), c["row_bytes"]), dtype=np.uint8)
    out[ok] = read_rows(source, c, source_offsets(rows[ok], n, c["step_pitch"], c["game_pitch"]))
    return out


def copy_bytes(source, c, n):
    return read_rows(source, c, np.arange(n, dtype=np.int64) * c["game_pitch"])


# ---- the shapes of the GPU test ------------------------------------------------------------------------------------------------
def basic_shapes():
    """(k, n, minibatches): n in {1, 63, 64, 65, 241} x k in {1, 2, 17} x minibatches in {1, 3, 4, M} where they fit.  M = 65
    and M = 4097 are the long walks (a domain of 256 and of 16384); B is a multiple of 64 (k = 1, 2, n = 64; 17 x 64 / 1) and
    not."""
    out = []
    for k in (1, 2, 17):
        for n in (1, 63, 64, 65, 241):
            M = k * n
            for mb in (1, 3, 4, M):
                if mb <= M and (k, n, mb) not in out:
                    out.append((k, n, mb))
    return out


def counters(minibatches):
    """the calls a shape is judged at: the first and the last minibatch of epoch 0, the second of epoch 1 and one of a far epoch"""
    return sorted({0, minibatches - 1, minibatches + min(1, minibatches - 1), (1 << 40) * minibatches + minibatches // 2})
