"""TensorBoard event files without TensorBoard: a pure-Python reader and the SummaryWriter binding.

read_events(path) is the only way to look into a run on a machine that has no `tensorboard` package: it
walks the record framing (uint64 length, masked CRC-32C of the length, payload, masked CRC-32C of the
payload), verifies both checksums, and decodes the protobuf wire format of Event / Summary by hand —
scalars, histograms, images (encoded bytes) and text; everything it does not know is kept as raw bytes.
It imports neither torch nor the shared library.

SummaryWriter(logdir) writes the same files through the C ABI (cad_tb_* in include/cad/cad.h, host only);
add_histograms(model, ...) takes its rows from the device histogram pass (cad_unet_histograms).
"""
from __future__ import annotations

import struct
from typing import Iterator, List, NamedTuple, Optional

__all__ = ["read_events", "Event", "Value", "Histogram", "Image", "EventFileError", "crc32c", "masked_crc32c",
           "default_bins", "trim_histogram", "SummaryWriter"]


class EventFileError(ValueError):
    """A record whose length or payload checksum does not match, or a payload that is not wire format."""


# ---------------------------------------------------------------- CRC-32C (Castagnoli, reflected 0x82F63B78)
def _make_table():
    t = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
        t.append(c)
    return t


_TABLE = _make_table()


def crc32c(data: bytes, crc: int = 0) -> int:
    c = crc ^ 0xFFFFFFFF
    t = _TABLE
    for b in bytes(data):
        c = t[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def masked_crc32c(data: bytes) -> int:
    c = crc32c(data)
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


# ---------------------------------------------------------------- protobuf wire format
def _varint(buf: bytes, i: int):
    x = 0
    shift = 0
    while True:
        if i >= len(buf) or shift > 63:
            raise EventFileError("truncated or overlong varint")
        b = buf[i]
        i += 1
        x |= (b & 0x7F) << shift
        if not b & 0x80:
            return x & 0xFFFFFFFFFFFFFFFF, i
        shift += 7


def _fields(buf: bytes):
    """(field number, wire type, value, raw bytes of the whole field) of one message."""
    i, n = 0, len(buf)
    while i < n:
        s = i
        key, i = _varint(buf, i)
        num, wt = key >> 3, key & 7
        if wt == 0:
            v, i = _varint(buf, i)
        elif wt == 1:
            v, i = buf[i:i + 8], i + 8
        elif wt == 5:
            v, i = buf[i:i + 4], i + 4
        elif wt == 2:
            ln, i = _varint(buf, i)
            v, i = buf[i:i + ln], i + ln
        else:
            raise EventFileError(f"unsupported wire type {wt}")
        if i > n:
            raise EventFileError("field runs past the end of its message")
        yield num, wt, v, buf[s:i]


def _doubles(wt: int, v: bytes) -> List[float]:
    if wt == 1:
        return [struct.unpack("<d", v)[0]]
    if len(v) % 8:
        raise EventFileError("packed doubles: length is no multiple of 8")
    return list(struct.unpack(f"<{len(v) // 8}d", v))


class Histogram(NamedTuple):
    min: float
    max: float
    num: float
    sum: float
    sum_squares: float
    bucket_limit: List[float]
    bucket: List[float]


class Image(NamedTuple):
    height: int
    width: int
    colorspace: int
    encoded: bytes


class Value(NamedTuple):
    tag: str
    kind: str                 # "scalar" | "histogram" | "image" | "text" | "tensor" | "unknown"
    value: object             # float | Histogram | Image | str | dict (tensor) | None
    plugin_name: str          # metadata.plugin_data.plugin_name ("" without metadata)
    plugin_content: bytes     # metadata.plugin_data.content
    metadata: bytes           # the SummaryMetadata message, raw
    unknown: list             # [(field number, wire type, raw value)] of fields not decoded


class Event(tuple):
    """(wall_time, step, [values]) of one record — a 3-tuple, with the rest of the record as attributes:
    file_version (the first record's), unknown (Event fields not decoded, ((field number, wire type, raw
    value), ...)) and payload (the record's payload as stored)."""

    def __new__(cls, wall_time: float, step: int, values: List[Value], file_version: Optional[str] = None,
                unknown: tuple = (), payload: bytes = b""):
        self = super().__new__(cls, (wall_time, step, values))
        self.file_version, self.unknown, self.payload = file_version, unknown, payload
        return self

    wall_time = property(lambda self: self[0])
    step = property(lambda self: self[1])
    values = property(lambda self: self[2])


def _parse_hist(buf: bytes) -> Histogram:
    d = {1: 0.0, 2: 0.0, 3: 0.0, 4: 0.0, 5: 0.0}
    lim: List[float] = []
    cnt: List[float] = []
    for num, wt, v, _ in _fields(buf):
        if num in d and wt == 1:
            d[num] = struct.unpack("<d", v)[0]
        elif num == 6:
            lim += _doubles(wt, v)
        elif num == 7:
            cnt += _doubles(wt, v)
    return Histogram(d[1], d[2], d[3], d[4], d[5], lim, cnt)


def _parse_image(buf: bytes) -> Image:
    h = w = cs = 0
    enc = b""
    for num, wt, v, _ in _fields(buf):
        if num == 1 and wt == 0:
            h = v
        elif num == 2 and wt == 0:
            w = v
        elif num == 3 and wt == 0:
            cs = v
        elif num == 4 and wt == 2:
            enc = bytes(v)
    return Image(h, w, cs, enc)


def _parse_tensor(buf: bytes) -> dict:
    t = {"dtype": 0, "shape": [], "string_val": [], "float_val": [], "tensor_content": b"", "unknown": []}
    for num, wt, v, _ in _fields(buf):
        if num == 1 and wt == 0:
            t["dtype"] = v
        elif num == 2 and wt == 2:
            for n2, w2, v2, _ in _fields(v):
                if n2 == 2 and w2 == 2:
                    t["shape"].append(next((x for k, w3, x, _ in _fields(v2) if k == 1 and w3 == 0), 0))
        elif num == 8 and wt == 2:
            t["string_val"].append(bytes(v))
        elif num == 5:
            t["float_val"] += ([struct.unpack("<f", v)[0]] if wt == 5 else list(struct.unpack(f"<{len(v) // 4}f", v)))
        elif num == 4 and wt == 2:
            t["tensor_content"] = bytes(v)
        else:
            t["unknown"].append((num, wt, bytes(v) if wt != 0 else v))
    return t


def _parse_value(buf: bytes) -> Value:
    tag, kind, val = "", "unknown", None
    plugin, content, meta = "", b"", b""
    unknown = []
    for num, wt, v, _ in _fields(buf):
        if num == 1 and wt == 2:
            tag = bytes(v).decode("utf-8", errors="replace")
        elif num == 2 and wt == 5:
            kind, val = "scalar", struct.unpack("<f", v)[0]
        elif num == 4 and wt == 2:
            kind, val = "image", _parse_image(v)
        elif num == 5 and wt == 2:
            kind, val = "histogram", _parse_hist(v)
        elif num == 8 and wt == 2:
            kind, val = "tensor", _parse_tensor(v)
        elif num == 9 and wt == 2:
            meta = bytes(v)
            for n2, w2, v2, _ in _fields(v):
                if n2 == 1 and w2 == 2:
                    for n3, w3, v3, _ in _fields(v2):
                        if n3 == 1 and w3 == 2:
                            plugin = bytes(v3).decode("utf-8", errors="replace")
                        elif n3 == 2 and w3 == 2:
                            content = bytes(v3)
        else:
            unknown.append((num, wt, bytes(v) if wt != 0 else v))
    if kind == "tensor" and plugin == "text" and val["string_val"]:
        kind, val = "text", val["string_val"][0].decode("utf-8", errors="replace")
    return Value(tag, kind, val, plugin, content, meta, unknown)


def parse_event(payload: bytes) -> Event:
    """Decode one record's payload (an Event message)."""
    wall, step, fv = 0.0, 0, None
    values: List[Value] = []
    unknown = []
    for num, wt, v, _ in _fields(payload):
        if num == 1 and wt == 1:
            wall = struct.unpack("<d", v)[0]
        elif num == 2 and wt == 0:
            step = v - (1 << 64) if v >> 63 else v
        elif num == 3 and wt == 2:
            fv = bytes(v).decode("utf-8", errors="replace")
        elif num == 5 and wt == 2:
            for n2, w2, v2, _ in _fields(v):
                if n2 == 1 and w2 == 2:
                    values.append(_parse_value(v2))
        else:
            unknown.append((num, wt, bytes(v) if wt != 0 else v))
    return Event(wall, step, values, fv, tuple(unknown), bytes(payload))


def read_records(path: str) -> Iterator[bytes]:
    """The payloads of an event file.  Raises EventFileError on a checksum mismatch; an incomplete last
    record (a live run is always mid-write) ends the iteration quietly."""
    with open(path, "rb") as fh:
        data = fh.read()
    i, n = 0, len(data)
    while i < n:
        if i + 12 > n:
            return
        head = data[i:i + 8]
        (ln,) = struct.unpack("<Q", head)
        (hc,) = struct.unpack("<I", data[i + 8:i + 12])
        if hc != masked_crc32c(head):
            raise EventFileError(f"{path}: length checksum mismatch at byte {i}")
        if i + 12 + ln + 4 > n:
            return
        payload = data[i + 12:i + 12 + ln]
        (pc,) = struct.unpack("<I", data[i + 12 + ln:i + 16 + ln])
        if pc != masked_crc32c(payload):
            raise EventFileError(f"{path}: payload checksum mismatch in the record at byte {i}")
        yield payload
        i += 16 + ln


def read_events(path: str) -> Iterator[Event]:
    """Yield (wall_time, step, [values]) per record of an event file (Event is that tuple, plus
    file_version, the undecoded Event fields and the raw payload)."""
    for payload in read_records(path):
        yield parse_event(payload)


def strip_wall_time(payload: bytes) -> bytes:
    """The payload without its Event.wall_time field (for comparing files written at different times)."""
    return b"".join(raw for num, wt, _, raw in _fields(payload) if not (num == 1 and wt == 1))


# ---------------------------------------------------------------- histogram buckets
def default_bins() -> List[float]:
    """TensorBoard's default bucket edges as torch.utils.tensorboard.writer builds them, in double."""
    v = 1e-12
    buckets = []
    while v < 1e20:
        buckets.append(v)
        v *= 1.1
    return [-x for x in reversed(buckets)] + [0.0] + buckets


def _abi_mod():
    from . import _abi          # lazy: the reader above needs neither ctypes nor the shared library
    return _abi


def trim_histogram(counts, edges=None):
    """make_histogram's trimming (torch/utils/tensorboard/summary.py) by the library: (bucket_limit, bucket)
    lists — first through last non-empty bucket plus one empty bucket on the left; (0, 0) when all are empty."""
    import ctypes as C

    import numpy as np
    _abi = _abi_mod()
    lib = _abi.load()
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    edges = np.ascontiguousarray(default_bins() if edges is None else edges, dtype=np.float64)
    if edges.size != counts.size + 1:
        raise ValueError("edges must have one more entry than counts")
    lim = np.empty(counts.size + 1, np.float64)
    buc = np.empty(counts.size + 1, np.float64)
    n = C.c_int()
    _abi.check(lib.cad_tb_trim_histogram(counts.ctypes.data_as(C.POINTER(C.c_uint32)), counts.size, edges.ctypes.data_as(_abi.DP),
                                         lim.ctypes.data_as(_abi.DP), buc.ctypes.data_as(_abi.DP), C.byref(n)), "trim_histogram")
    return lim[:n.value].tolist(), buc[:n.value].tolist()


class SummaryWriter:
    """torch.utils.tensorboard.SummaryWriter's surface for what the trainer logs, over cad_tb_* (cad.h).
    Every writer opens a new event file under logdir; nothing here touches the device except
    add_histograms, which runs the model's histogram pass."""

    def __init__(self, logdir: str):
        import ctypes as C
        self._abi = _abi_mod()
        self.lib = self._abi.load()
        self.logdir = str(logdir)
        h = C.c_void_p()
        self._abi.check(self.lib.cad_tb_open(self.logdir.encode(), C.byref(h)), "cad_tb_open")
        self.h = h
        self._edges = None

    @property
    def path(self) -> str:
        return self.lib.cad_tb_path(self._handle()).decode()

    @property
    def hparams_path(self) -> str:
        return self.lib.cad_tb_hparams_path(self._handle()).decode()

    def _handle(self):
        if self.h is None:
            raise ValueError("the writer is closed")
        return self.h

    def add_scalar(self, tag: str, value: float, step: int = 0):
        self._abi.check(self.lib.cad_tb_scalar(self._handle(), tag.encode(), float(value), int(step)), "cad_tb_scalar")

    def add_histogram_raw(self, tag, min, max, num, sum, sum_squares, bucket_limits, bucket_counts, step=0):
        import ctypes as C

        import numpy as np
        lim = np.ascontiguousarray(bucket_limits, dtype=np.float64)
        buc = np.ascontiguousarray(bucket_counts, dtype=np.float64)
        if lim.size != buc.size:
            raise ValueError("bucket_limits and bucket_counts differ in length")
        stats = (C.c_double * 5)(min, max, num, sum, sum_squares)
        self._abi.check(self.lib.cad_tb_histogram(self._handle(), tag.encode(), int(step), stats, lim.ctypes.data_as(self._abi.DP),
                                                  buc.ctypes.data_as(self._abi.DP), lim.size), "cad_tb_histogram")

    def add_histogram(self, tag: str, values, step: int = 0):
        """Histogram of a host array over the default buckets (numpy.histogram's rule, then the trimming)."""
        import numpy as np
        v = np.asarray(values).reshape(-1).astype(np.float64)
        v = v[np.isfinite(v)]
        if self._edges is None:
            self._edges = np.asarray(default_bins(), np.float64)
        counts, _ = np.histogram(v, bins=self._edges)
        lim, buc = trim_histogram(counts, self._edges)
        if v.size:
            self.add_histogram_raw(tag, v.min(), v.max(), v.size, v.sum(), float(v.dot(v)), lim, buc, step)
        else:
            self.add_histogram_raw(tag, 0.0, 0.0, 0, 0.0, 0.0, lim, buc, step)

    def add_histograms(self, model, prefix: str = "weights", which: str = "params", step: int = 0):
        """One histogram per named_parameters() entry from the device pass, tagged as the reference tags
        them: <prefix>/<name with '.' -> '/'> (prefix "weights" for which="params", "gradients" for "grads")."""
        for name, (st, counts) in model.histograms(which).items():
            lim, buc = trim_histogram(counts)
            self.add_histogram_raw(f"{prefix}/{name.replace('.', '/')}", st["min"], st["max"], st["num"], st["sum"],
                                   st["sum_squares"], lim, buc, step)

    def add_image(self, tag: str, image, step: int = 0):
        """image: an HWC (or HW) uint8 array, or the bytes of an encoded PNG."""
        import numpy as np
        if isinstance(image, (bytes, bytearray, memoryview)):
            from .export import decode_png
            png = bytes(image)
            arr = decode_png(png)
            h, w = arr.shape[:2]
            ch = 1 if arr.ndim == 2 else arr.shape[2]
        else:
            from .export import encode_png
            arr = np.ascontiguousarray(image)
            if arr.dtype != np.uint8 or arr.ndim not in (2, 3):
                raise ValueError("add_image needs an HWC / HW uint8 array or encoded PNG bytes")
            h, w = arr.shape[:2]
            ch = 1 if arr.ndim == 2 else arr.shape[2]
            png = encode_png(arr)
        self._abi.check(self.lib.cad_tb_image(self._handle(), tag.encode(), int(step), h, w, ch, png, len(png)), "cad_tb_image")

    def add_text(self, tag: str, text: str, step: int = 0):
        self._abi.check(self.lib.cad_tb_text(self._handle(), tag.encode(), int(step), text.encode()), "cad_tb_text")

    def add_custom_scalars(self, layout: dict):
        """layout: {category: {chart: [tags]}} (or {chart: ["Multiline", [tags]]} as torch takes it)."""
        import ctypes as C
        rows = []
        for cat, charts in layout.items():
            for chart, tags in charts.items():
                if len(tags) == 2 and isinstance(tags[0], str) and isinstance(tags[1], (list, tuple)):
                    if tags[0] != "Multiline":
                        raise ValueError("only Multiline charts are written")
                    tags = tags[1]
                rows += [(cat, chart, t) for t in tags]
        arr = lambda k: (C.c_char_p * max(len(rows), 1))(*[r[k].encode() for r in rows])
        self._abi.check(self.lib.cad_tb_custom_scalars(self._handle(), arr(0), arr(1), arr(2), len(rows)), "cad_tb_custom_scalars")

    def add_hparams(self, hparams: dict, metrics: dict, run_name: str | None = None):
        import ctypes as C
        names = (C.c_char_p * max(len(hparams), 1))(*[k.encode() for k in hparams])
        vals = (C.c_double * max(len(hparams), 1))(*[float(v) for v in hparams.values()])
        mt = (C.c_char_p * max(len(metrics), 1))(*[k.encode() for k in metrics])
        mv = (C.c_float * max(len(metrics), 1))(*[float(v) for v in metrics.values()])
        self._abi.check(self.lib.cad_tb_hparams(self._handle(), names, vals, len(hparams), mt, mv, len(metrics),
                                                run_name.encode() if run_name else None), "cad_tb_hparams")

    def flush(self):
        self._abi.check(self.lib.cad_tb_flush(self._handle()), "cad_tb_flush")

    def close(self):
        if self.h is not None:
            self.lib.cad_tb_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
