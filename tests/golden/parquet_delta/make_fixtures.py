"""Writes the fixtures of this directory; needed only to make them again (it needs pyarrow; the tests read the files).

pyarrow writes nullable columns of 5000 rows, not dictionary-encoded and uncompressed, under data_page_version "1.0" and
"2.0", through column_encoding=: every seventh row and rows 2000 to 2299 are null.
  sums64   int64, DELTA_BINARY_PACKED: ascending sums of steps below 1000, every 50th step negative
  int32    int32, DELTA_BINARY_PACKED: a random walk with steps of up to 16 bits either way
  const    int64, DELTA_BINARY_PACKED: one value, so every width is 0
  wrap64   int64, DELTA_BINARY_PACKED: its minimum and its maximum in turn, so every delta wraps
  strings  string, DELTA_LENGTH_BYTE_ARRAY: lengths 0 to 8, empty strings among them
Per file <version>_<column>.bin and .json: every data page's definition-level stream and value stream (everything of
the page behind the levels) as they lie in the file, and what they hold -- pinned to the table pyarrow was given (a
level of 1 where the row is not null; the row's values in 4 or 8 bytes each, or the Arrow offsets in 4 bytes each and
the strings' bytes), not to any decoder of delta streams.  The json also records the block size and the miniblocks per
block that the first bytes of each value stream say."""
import io
import json
import os
import struct
import sys

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import parquet_pagegen as P  # noqa: E402

ROWS = 5000
DELTA_BINARY_PACKED, DELTA_LENGTH_BYTE_ARRAY = 5, 6


def columns():
    rng = np.random.default_rng(28)
    steps = [int(s) for s in rng.integers(0, 1000, ROWS)]
    sums, at = [], -123456789
    for i, s in enumerate(steps):
        at += -s if i % 50 == 49 else s
        sums.append(at)
    walk, at = [], 1000
    for s in rng.integers(-65535, 65536, ROWS):
        at += int(s)
        walk.append(at)
    ends = (-(1 << 63), (1 << 63) - 1)
    letters = "abcdefghijklmnopqrstuvwxyz"
    strings = ["".join(letters[int(c)] for c in rng.integers(0, 26, int(n))) for n in rng.integers(0, 9, ROWS)]
    return {"sums64": (pa.int64(), sums, "DELTA_BINARY_PACKED", 8),
            "int32": (pa.int32(), walk, "DELTA_BINARY_PACKED", 4),
            "const": (pa.int64(), [77] * ROWS, "DELTA_BINARY_PACKED", 8),
            "wrap64": (pa.int64(), [ends[i % 2] for i in range(ROWS)], "DELTA_BINARY_PACKED", 8),
            "strings": (pa.string(), strings, "DELTA_LENGTH_BYTE_ARRAY", 0)}


def varints(data, count):
    out, pos = [], 0
    for _ in range(count):
        v = n = 0
        while True:
            b = data[pos]
            pos += 1
            v |= (b & 0x7F) << (7 * n)
            n += 1
            if not b & 0x80:
                break
        out.append(v)
    return out


def main():
    for version in ("1.0", "2.0"):
        for column, (kind, values, encoding, element) in columns().items():
            rows = [None if i % 7 == 0 or 2000 <= i < 2300 else v for i, v in enumerate(values)]
            sink = io.BytesIO()
            pq.write_table(pa.table({"c": pa.array(rows, kind)}), sink, use_dictionary=False, compression="none",
                           column_encoding={"c": encoding}, data_page_version=version, data_page_size=1024, write_batch_size=128)
            data = sink.getvalue()
            col = pq.ParquetFile(io.BytesIO(data)).metadata.row_group(0).column(0)
            assert not col.has_dictionary_page
            chunk = data[col.data_page_offset:col.data_page_offset + col.total_compressed_size]
            pages = P.walk(chunk, P.UNCOMPRESSED)
            blob, listed, row = bytearray(), [], 0

            def put(b):
                at = len(blob)
                blob.extend(b)
                return [at, len(b)]

            for p in pages:
                assert p["encoding"] == (DELTA_BINARY_PACKED if element else DELTA_LENGTH_BYTE_ARRAY), "a page fell back"
                body = chunk[p["body_offset"]:p["body_offset"] + p["compressed_page_size"]]
                if p["kind"] == P.DATA_PAGE_V2:
                    assert p["rep_levels_bytes"] == 0
                    levels = p["def_levels_bytes"]
                else:
                    assert p["kind"] == P.DATA_PAGE
                    levels = 4 + struct.unpack_from("<I", body)[0]
                mine = rows[row:row + p["num_values"]]
                row += p["num_values"]
                there = [v for v in mine if v is not None]
                block, miniblocks = varints(body[levels:], 2)
                entry = dict(num_values=p["num_values"], non_null=len(there), block_size=block, miniblocks=miniblocks,
                             level_stream=put(body[:levels]), value_stream=put(body[levels:]),
                             expected_levels=put(bytes(v is not None for v in mine)))
                if element:
                    entry["expected_values"] = put(struct.pack("<%d%s" % (len(there), "i" if element == 4 else "q"), *there))
                else:
                    offsets = [0]
                    for s in there:
                        offsets.append(offsets[-1] + len(s.encode()))
                    entry["expected_offsets"] = put(struct.pack("<%di" % len(offsets), *offsets))
                    entry["expected_bytes"] = put("".join(there).encode())
                listed.append(entry)
            assert row == ROWS and listed and len(blob) < 65536, (column, len(blob))   # (const and wrap64: one page holds all rows)
            name = "v%s_%s" % (version[0], column)
            with open(os.path.join(HERE, name + ".bin"), "wb") as f:
                f.write(blob)
            with open(os.path.join(HERE, name + ".json"), "w") as f:
                json.dump(dict(pyarrow=pa.__version__, data_page_version=version, column=column, encoding=encoding,
                               element_bytes=element, pages=listed), f, indent=1)
                f.write("\n")
            print(name, len(blob), "bytes,", len(listed), "pages, block", sorted({(p["block_size"], p["miniblocks"]) for p in listed}))


if __name__ == "__main__":
    main()
