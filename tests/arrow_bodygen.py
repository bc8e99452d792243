"""Arrow IPC record-batch bodies with LZ4-compressed buffers, as fixtures for decompress_frames of the LZ4 manager
(hipcomp/lz4.hpp, LZ4FramePrefix::ArrowLength; INTEGRATION.md, "Batches of LZ4 frames").

A body is the buffers of a record batch one after the other, each padded to 8 bytes; a compressed buffer is an
8-byte little-endian length -- the decoded size, or -1 for "the bytes behind this are the buffer itself" -- and one
LZ4 frame.  Where the buffers stand is written in the flatbuffer metadata in front of the body; this module does not
read that.  It finds them by walking the body: prefix, the frame's block chain to its EndMark, pad to 8 -- which must
end exactly at the body's length -- and holds every decoded size to the matching column.buffers() entry.

  record_batch_body()   what pyarrow writes for a small batch with IpcWriteOptions(compression="lz4")
  codec_body()          a body put together here from pa.Codec("lz4") frames, with a stored (-1) and an empty item
Both need pyarrow.  `python tests/arrow_bodygen.py` writes them to tests/golden/arrow_ipc/ as <name>.body and
<name>.json: {"body_sha256", "items": [{"offset", "length", "decoded_size", "sha256", "stored"}]}, length 0 for an
empty item.  The tests read the committed files and need no pyarrow."""
import hashlib
import json
import os
import struct

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "arrow_ipc")
ROWS = 20000
MAGIC = 0x184D2204


def frame_end(buf: bytes, at: int) -> int:
    """the offset behind the LZ4 frame that starts at buf[at]: header, block chain, EndMark, content checksum"""
    magic, flg = struct.unpack_from("<IB", buf, at)
    assert magic == MAGIC and flg >> 6 == 1, "not an LZ4 frame"
    at += 7 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
    while True:
        word, = struct.unpack_from("<I", buf, at)
        at += 4
        if word & 0x7FFFFFFF == 0:
            return at + (4 if flg & 4 else 0)
        at += (word & 0x7FFFFFFF) + (4 if flg & 0x10 else 0)


def walk(body: bytes):
    """[(offset, length, prefix)] of the compressed buffers of a body pyarrow wrote (none of them stored)"""
    items, at = [], 0
    while at < len(body):
        p, = struct.unpack_from("<q", body, at)
        assert p >= 0, "a stored buffer: its length is in the metadata alone"
        end = frame_end(body, at + 8)
        items.append((at, end - at, p))
        at = (end + 7) & ~7
    assert at == len(body), "the walk does not end at the body's end"
    return items


def _runs(rng, values, mean):
    """ROWS values drawn from `values`, each repeated a random number of times around `mean`: compressible columns keep
    the committed body small while every buffer still has the blocks its size gives it"""
    out = []
    while len(out) < ROWS:
        out += [values[rng.integers(0, len(values))]] * int(rng.integers(1, 2 * mean))
    return out[:ROWS]


def _table():
    """int64 ramp, low-cardinality int32, strings, doubles, nullable int16: the 8-byte columns are 160 000 bytes (three
    linked 64 KiB blocks), the int32 column and the strings' offsets 80 000 (two), the validity bitmap is one block"""
    import pyarrow as pa
    rng = np.random.default_rng(25)
    words = ["lineitem", "orders", "customer", "part", "supplier", "nation", "region", "partsupp", ""]
    strings = [w if rng.integers(0, 4) == 0 else "" for w in _runs(rng, words, 14)]
    return pa.table({
        "ramp": pa.array(np.arange(ROWS, dtype=np.int64) // 16),
        "low_cardinality": pa.array(np.array(_runs(rng, [0, 1, 2, 3, 4], 20), dtype=np.int32)),
        "strings": pa.array(strings),
        "doubles": pa.array(np.array(_runs(rng, [0.25 * k for k in range(16)], 10), dtype=np.float64)),
        "nullable": pa.array(np.array(_runs(rng, list(range(-5, 5)), 10), dtype=np.int16), mask=rng.integers(0, 8, ROWS) == 0),
    })


def record_batch_body():
    """(body, items): items as in the manifest, held to the columns' own buffers"""
    import pyarrow as pa
    batch = _table().combine_chunks().to_batches()[0]
    sink = pa.BufferOutputStream()
    with pa.ipc.new_stream(sink, batch.schema, options=pa.ipc.IpcWriteOptions(compression="lz4")) as w:
        w.write_batch(batch)
    messages = list(pa.ipc.MessageReader.open_stream(sink.getvalue()))
    body = [m for m in messages if m.type == "record batch"][0].body.to_pybytes()
    buffers = [b for col in batch.columns for b in col.buffers() if b is not None and b.size > 0]
    found = walk(body)
    assert len(found) == len(buffers), (len(found), len(buffers))
    codec, items = pa.Codec("lz4"), []
    for (offset, length, p), buf in zip(found, buffers):
        data = codec.decompress(body[offset + 8:offset + length], p).to_pybytes()
        assert len(data) == p == buf.size and data == buf.to_pybytes(), "the buffer is not the column's"
        items.append({"offset": offset, "length": length, "decoded_size": p, "sha256": hashlib.sha256(data).hexdigest(),
                      "stored": False})
    return body, items


def codec_body():
    """frames of pa.Codec("lz4") behind prefixes written here: text of three blocks, noise (stored blocks), a short
    buffer, a buffer stored whole (-1), an empty item (no bytes at all), one more frame behind it"""
    import pyarrow as pa
    rng = np.random.default_rng(7)
    codec = pa.Codec("lz4")
    text = b" ".join(b"%s|%d|1996-%02d-%02d" % (w, k * k, 1 + k % 12, 1 + k % 28)
                     for k, w in enumerate([b"furiously", b"regular", b"deposits", b"sleep", b"blithely"] * 2400))[:135000]
    plan = [("text", text, False), ("noise", rng.integers(0, 256, 3000, dtype=np.uint8).tobytes(), False),
            ("short", b"arrow", False), ("stored", rng.integers(0, 256, 333, dtype=np.uint8).tobytes(), True),
            ("empty", b"", None), ("zeros", bytes(70000), False)]
    body, items = bytearray(), []
    for _, data, stored in plan:
        if stored is None:
            piece = b""
        elif stored:
            piece = struct.pack("<q", -1) + data
        else:
            piece = struct.pack("<q", len(data)) + codec.compress(data).to_pybytes()
        items.append({"offset": len(body), "length": len(piece), "decoded_size": len(data),
                      "sha256": hashlib.sha256(data).hexdigest(), "stored": bool(stored)})
        body += piece + bytes(-len(piece) % 8)
    return bytes(body), items


def write(name, body, items):
    os.makedirs(GOLDEN, exist_ok=True)
    with open(os.path.join(GOLDEN, name + ".body"), "wb") as f:
        f.write(body)
    with open(os.path.join(GOLDEN, name + ".json"), "w") as f:
        json.dump({"body_sha256": hashlib.sha256(body).hexdigest(), "items": items}, f, indent=1)
        f.write("\n")


def load(name):
    """(body, items) of a committed fixture"""
    body = open(os.path.join(GOLDEN, name + ".body"), "rb").read()
    m = json.load(open(os.path.join(GOLDEN, name + ".json")))
    assert hashlib.sha256(body).hexdigest() == m["body_sha256"], name
    return body, m["items"]


FIXTURES = ("record_batch", "codec")

if __name__ == "__main__":
    write("record_batch", *record_batch_body())
    write("codec", *codec_body())
    for n in FIXTURES:
        b, it = load(n)
        print(n, len(b), "bytes,", len(it), "items")
