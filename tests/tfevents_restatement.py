"""Yardsticks of the TensorBoard tests, in numpy: the default buckets and make_histogram of
torch/utils/tensorboard (writer.py's default_bins loop, summary.py's start / end rule), and a bitwise
CRC-32C.  Nothing here calls the library under test."""
import numpy as np


def default_bins():
    v = 1e-12
    buckets, neg = [], []
    while v < 1e20:
        buckets.append(v)
        neg.append(-v)
        v *= 1.1
    return np.asarray(neg[::-1] + [0] + buckets, np.float64)


def counts_of(values, edges=None):
    """numpy.histogram of the values widened to double over the default edges."""
    edges = default_bins() if edges is None else edges
    counts, _ = np.histogram(np.asarray(values).reshape(-1).astype(np.float64), bins=edges)
    return counts


def trim(counts, limits):
    """make_histogram's support rule: (bucket_limit, bucket).  All-empty counts (where make_histogram itself
    raises) give the single pair (0, 0), the project's documented rule."""
    counts = np.asarray(counts)
    if not np.any(counts > 0):
        return [0.0], [0.0]
    cum_counts = np.cumsum(np.greater(counts, 0))
    start, end = np.searchsorted(cum_counts, [0, cum_counts[-1] - 1], side="right")
    start = int(start)
    end = int(end) + 1
    counts = counts[start - 1:end] if start > 0 else np.concatenate([[0], counts[:end]])
    limits = limits[start:end + 1]
    return [float(x) for x in limits], [float(x) for x in counts]


def make_histogram(values):
    """(min, max, num, sum, sum_squares, bucket_limit, bucket) of finite values, all in float64."""
    v = np.asarray(values).reshape(-1).astype(np.float64)
    edges = default_bins()
    lim, buc = trim(counts_of(v, edges), edges)
    return float(v.min()), float(v.max()), float(v.size), float(v.sum()), float(v.dot(v)), lim, buc


def crc32c_bitwise(data: bytes) -> int:
    """CRC-32C one bit at a time (reflected polynomial 0x82F63B78): slow and plain."""
    c = 0xFFFFFFFF
    for b in data:
        c ^= b
        for _ in range(8):
            c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
    return c ^ 0xFFFFFFFF
