"""TensorBoard event files without a GPU: CRC-32C, the pure-Python reader on the two files the reference's
run left (tests/golden/tfevents), the native writer against those files byte for byte, round trips of the
record kinds the fixtures do not hold, and the histogram trimming against make_histogram's rule
(tests/tfevents_restatement.py)."""
import ctypes as C
import glob
import os
import struct

import numpy as np
import pytest

import tfevents_restatement as R
from conftest import GOLDEN

FIX = os.path.join(GOLDEN, "tfevents")
MAIN = os.path.join(FIX, "events.out.tfevents.1766492499.Reiyos-MacBook-Pro.local.71017.0")
SUB = os.path.join(FIX, "1766492499.256311", "events.out.tfevents.1766492499.Reiyos-MacBook-Pro.local.71017.1")


@pytest.fixture(scope="module")
def tb(cad):
    from cad_amd import tbevents
    return tbevents


# ---------------------------------------------------------------- 1. CRC
def test_crc32c_vectors(cad, tb):
    lib = cad.load_library()
    for crc in (lambda b: lib.cad_crc32c(b, len(b)), tb.crc32c):
        assert crc(b"123456789") == 0xE3069283
        assert crc(b"") == 0
        assert crc(b"\x00" * 32) == 0x8A9136AA          # RFC 3720 B.4
        assert crc(b"\xff" * 32) == 0x62A8AB43
    rng = np.random.default_rng(7)
    big = rng.integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
    want = R.crc32c_bitwise(big)
    assert lib.cad_crc32c(big, len(big)) == want
    assert tb.crc32c(big) == want


def test_crc_mask_formula(cad, tb):
    lib = cad.load_library()
    c = 0xE3069283
    want = (((c >> 15) | (c << 17)) + 0xA282EAD8) % (1 << 32)
    assert lib.cad_crc32c_masked(b"123456789", 9) == want == tb.masked_crc32c(b"123456789")
    # a known pair from a file TensorBoard's writer produced: the first record's length field and its checksum
    data = open(MAIN, "rb").read()
    assert lib.cad_crc32c_masked(data[:8], 8) == struct.unpack("<I", data[8:12])[0]


# ---------------------------------------------------------------- 2. reader on the reference's files
def test_reader_on_reference_files(tb):
    main = list(tb.read_events(MAIN))
    sub = list(tb.read_events(SUB))
    assert len(main) == 13 and len(sub) == 5
    assert main[0].file_version == "brain.Event:2" and sub[0].file_version == "brain.Event:2"
    assert not main[0].values
    kinds = [(v.tag, v.kind, v.plugin_name) for e in main for v in e.values]
    assert kinds[0] == ("custom_scalars__config__", "tensor", "custom_scalars")
    assert kinds[1] == ("model/architecture/text_summary", "text", "text")
    assert kinds[2:] == [("batch_loss/train", "scalar", ""), ("training/gradient_norm", "scalar", "")] * 5
    assert [e.step for e in main[3:]] == [9, 9, 19, 19, 29, 29, 39, 39, 49, 49]
    wall, step, values = main[3]                      # the documented (wall_time, step, [values]) shape
    assert step == 9 and wall > 1.7e9
    assert values[0].tag == "batch_loss/train" and values[0].value == float(np.float32(1.2563012838363647))
    assert "Total parameters: 31037633" in main[2].values[0].value
    assert [(v.tag, v.kind, v.plugin_name) for e in sub for v in e.values] == [
        ("_hparams_/experiment", "unknown", "hparams"), ("_hparams_/session_start_info", "unknown", "hparams"),
        ("_hparams_/session_end_info", "unknown", "hparams"), ("hparams/training", "scalar", "")]
    assert sub[1].values[0].plugin_content            # unknown fields are kept as raw bytes
    assert sub[4].values[0].value == 0.0 and sub[4].step == 0


def test_reader_rejects_a_flipped_byte(tb, tmp_path):
    data = bytearray(open(MAIN, "rb").read())
    (ln,) = struct.unpack("<Q", data[:8])
    for pos in (12 + ln // 2, 3, 12 + 16 + ln + 20):    # first payload, first length, second record's payload
        bad = bytearray(data)
        bad[pos] ^= 0x10
        p = tmp_path / f"bad{pos}"
        p.write_bytes(bad)
        with pytest.raises(tb.EventFileError):
            list(tb.read_events(str(p)))


def test_reader_stops_at_an_incomplete_record(tb, tmp_path):
    data = open(MAIN, "rb").read()
    whole = list(tb.read_events(MAIN))
    for cut in (len(data) - 1, len(data) - 4, len(data) - 20, len(data) - len(whole[-1].payload) - 10):
        p = tmp_path / f"cut{cut}"
        p.write_bytes(data[:cut])
        got = list(tb.read_events(str(p)))
        assert [e.payload for e in got] == [e.payload for e in whole[:-1]]


# ---------------------------------------------------------------- 3. writer against the fixtures, byte for byte
def _layout_rows(tb, layout: bytes):
    """(category, chart, tag) rows of a custom_scalars Layout message."""
    rows = []
    for n1, w1, cat, _ in tb._fields(layout):
        assert (n1, w1) == (2, 2)
        title, charts = None, []
        for n2, w2, v2, _ in tb._fields(cat):
            if n2 == 1:
                title = bytes(v2).decode()
            else:
                assert (n2, w2) == (2, 2)
                charts.append(v2)
        for ch in charts:
            ctitle = None
            for n3, w3, v3, _ in tb._fields(ch):
                if n3 == 1:
                    ctitle = bytes(v3).decode()
                else:
                    assert (n3, w3) == (2, 2), "only multiline charts in the fixture"
                    rows += [(title, ctitle, bytes(t).decode()) for n4, _, t, _ in tb._fields(v3) if n4 == 1]
    return rows


def _hparams_of(tb, events):
    """{name: float64} of the session_start_info record and the metric tags of the experiment record."""
    hp = {}
    (start,) = [f for f in tb._fields(events[2].values[0].plugin_content)]
    assert start[0] == 3
    for n, _, entry, _ in tb._fields(start[2]):
        assert n == 1
        d = {k: v for k, _, v, _ in tb._fields(entry)}
        ((k2, w2, num, _),) = list(tb._fields(d[2]))
        assert (k2, w2) == (2, 1)
        hp[bytes(d[1]).decode()] = struct.unpack("<d", num)[0]
    return hp


def test_writer_reproduces_reference_records(cad, tb, tmp_path):
    main = list(tb.read_events(MAIN))
    sub = list(tb.read_events(SUB))
    rows = _layout_rows(tb, main[1].values[0].value["string_val"][0])
    assert ("Training", "Loss", "loss/train") in rows and len(rows) > 10
    layout = {}
    for cat, chart, tag in rows:
        layout.setdefault(cat, {}).setdefault(chart, []).append(tag)
    hp = _hparams_of(tb, sub)
    assert sorted(hp) == ["batch_size", "grad_clip_value", "learning_rate", "num_epochs", "weight_decay"]
    assert hp["learning_rate"] == float(np.float32(2e-4)) and hp["batch_size"] == 16.0

    w = tb.SummaryWriter(str(tmp_path / "run"))
    w.add_custom_scalars(layout)
    text = main[2].values[0]
    assert text.tag.endswith("/text_summary")
    w.add_text(text.tag[:-len("/text_summary")], text.value, main[2].step)
    for e in main[3:]:
        w.add_scalar(e.values[0].tag, e.values[0].value, e.step)
    # given in another order than the file's: the writer sorts hyper-parameters by name, as the map does
    w.add_hparams({k: hp[k] for k in sorted(hp, reverse=True)}, {"hparams/training": 0.0}, run_name="1766492499.256311")
    path, hpath = w.path, w.hparams_path
    w.close()
    assert os.path.dirname(hpath) == str(tmp_path / "run" / "1766492499.256311")
    for ours, ref in ((path, MAIN), (hpath, SUB)):
        a = [tb.strip_wall_time(p) for p in tb.read_records(ours)]
        b = [tb.strip_wall_time(p) for p in tb.read_records(ref)]
        assert len(a) == len(b)
        for i, (x, y) in enumerate(zip(a, b)):
            assert x == y, f"record {i} of {os.path.basename(ref)} differs"
    # and the framing itself: same record lengths, hence same file size
    assert os.path.getsize(path) == os.path.getsize(MAIN) == 1400
    assert os.path.getsize(hpath) == os.path.getsize(SUB) == 615


def test_file_name_and_fresh_file_per_writer(cad, tb, tmp_path):
    import socket
    d = tmp_path / "a" / "b"
    w1 = tb.SummaryWriter(str(d))
    w2 = tb.SummaryWriter(str(d))                       # a resume: a new file, never an append
    assert w1.path != w2.path
    name = os.path.basename(w1.path).split(".")
    assert name[:3] == ["events", "out", "tfevents"] and name[3].isdigit() and name[-1].isdigit()
    assert name[-2] == str(os.getpid()) and socket.gethostname() in os.path.basename(w1.path)
    w1.add_scalar("x", 1.0, 1)
    p1, p2 = w1.path, w2.path
    w1.close()
    w2.close()
    assert len(list(tb.read_events(p1))) == 2 and len(list(tb.read_events(p2))) == 1
    assert len(glob.glob(str(d / "events.out.tfevents.*"))) == 2


# ---------------------------------------------------------------- 4. round trip
def test_round_trip_histogram_image_and_edge_cases(cad, tb, tmp_path):
    w = tb.SummaryWriter(str(tmp_path))
    rng = np.random.default_rng(3)
    vals = (rng.standard_normal(5000) * 10.0 ** rng.uniform(-6, 3, 5000)).astype(np.float32)
    w.add_histogram("h/vals", vals, 7)
    img = rng.integers(0, 256, (5, 12, 3), dtype=np.uint8)
    w.add_image("img/a", img, 0)
    png = cad.encode_png(img[:, :, 0].copy())
    w.add_image("img/gray", png, 2)
    long_tag = "t" * 300
    w.add_scalar("", 1.5, 0)
    w.add_scalar(long_tag, -2.25, (1 << 32) + 5)
    w.add_scalar("s/big", 3.0, (1 << 62) + 1)
    w.add_scalar("s/nan", float("nan"), 1)
    w.add_scalar("s/inf", float("inf"), 2)
    w.add_scalar("s/ninf", float("-inf"), 3)
    w.add_text("note", "héllo\nworld", 4)
    w.flush()
    ev = list(tb.read_events(w.path))                   # readable while the writer is still open
    w.close()
    assert len(ev) == 11
    h = ev[1].values[0]
    assert (h.tag, h.kind, ev[1].step) == ("h/vals", "histogram", 7)
    mn, mx, num, sm, sq, lim, buc = R.make_histogram(vals)
    assert (h.value.min, h.value.max, h.value.num, h.value.sum, h.value.sum_squares) == (mn, mx, num, sm, sq)
    assert h.value.bucket_limit == lim and h.value.bucket == buc and sum(buc) == 5000
    im = ev[2].values[0]
    assert (im.tag, im.kind, ev[2].step) == ("img/a", "image", 0)
    assert (im.value.height, im.value.width, im.value.colorspace) == (5, 12, 3)
    assert np.array_equal(cad.decode_png(im.value.encoded), img)
    g = ev[3].values[0].value
    assert (g.height, g.width, g.colorspace) == (5, 12, 1) and g.encoded == png and ev[3].step == 2
    assert (ev[4].values[0].tag, ev[4].values[0].value, ev[4].step) == ("", 1.5, 0)
    assert (ev[5].values[0].tag, ev[5].values[0].value, ev[5].step) == (long_tag, -2.25, (1 << 32) + 5)
    assert ev[6].step == (1 << 62) + 1
    assert np.isnan(ev[7].values[0].value) and ev[8].values[0].value == np.inf and ev[9].values[0].value == -np.inf
    assert (ev[10].values[0].tag, ev[10].values[0].kind, ev[10].values[0].value) == ("note/text_summary", "text", "héllo\nworld")


# ---------------------------------------------------------------- 5. trimming
def _counts(pairs):
    c = np.zeros(len(R.default_bins()) - 1, np.uint32)
    for i, n in pairs:
        c[i] = n
    return c


@pytest.mark.parametrize("pairs", [
    [(400, 3), (401, 0), (402, 9), (1100, 1)],        # empty buckets at both ends and inside
    [(777, 5)],                                       # a single non-empty bucket
    [(0, 2), (5, 1)],                                 # the first bucket non-empty: start == 0
    [(0, 1)],
    [(1547, 4)],                                      # the last bucket
    [(0, 1), (1547, 1)],
    [],                                               # nothing in any bucket: the pair (0, 0)
])
def test_trimming_matches_make_histogram(cad, tb, pairs):
    lib = cad.load_library()
    n = lib.cad_tb_default_bins(None, 0)
    edges = np.empty(n, np.float64)
    assert lib.cad_tb_default_bins(edges.ctypes.data_as(C.POINTER(C.c_double)), n) == n
    ref_edges = R.default_bins()
    assert n == len(ref_edges) == 1549 and np.array_equal(edges, ref_edges)      # bit-equal doubles
    assert np.array_equal(np.asarray(tb.default_bins()), ref_edges)
    counts = _counts(pairs)
    lim, buc = tb.trim_histogram(counts)
    want_lim, want_buc = R.trim(counts, ref_edges)
    assert lim == want_lim and buc == want_buc
    if not pairs:
        assert (lim, buc) == ([0.0], [0.0])
    else:
        assert buc[0] == 0.0 and sum(buc) == sum(n for _, n in pairs)


def test_trimming_on_values(cad, tb):
    rng = np.random.default_rng(11)
    for vals in (rng.standard_normal(1000).astype(np.float32), np.ones(64, np.float32), np.zeros(9, np.float32),
                 np.asarray([-3e-13, 0.0, 2e-13], np.float32)):
        counts = R.counts_of(vals)
        lim, buc = tb.trim_histogram(counts.astype(np.uint32))
        _, _, _, _, _, want_lim, want_buc = R.make_histogram(vals)
        assert lim == want_lim and buc == want_buc
