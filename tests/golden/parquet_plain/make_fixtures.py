"""Writes the fixtures of this directory; needed only to make them again (it needs pyarrow; the tests read the files).

pyarrow writes nullable columns of 1500 rows, not dictionary-encoded (use_dictionary=False, column_encoding) and
uncompressed, under data_page_version "1.0" and "2.0": every seventh row and rows 600 to 999 are null, so one page at
least is wholly null; data_page_size is small and max_rows_per_page is 100, so a chunk has several data pages.
  column      type                                             encoding                  value bytes
  int32       int32                                            PLAIN                     4
  int64       int64                                            PLAIN                     8
  float       float32                                          PLAIN, BYTE_STREAM_SPLIT  4
  double      float64                                          PLAIN, BYTE_STREAM_SPLIT  8
  int96       timestamp[ns], use_deprecated_int96_timestamps   PLAIN                     12
  decimal5    decimal128(11, 2), FIXED_LEN_BYTE_ARRAY of 5     PLAIN                     5
  decimal16   decimal128(38, 4), FIXED_LEN_BYTE_ARRAY of 16    PLAIN                     16
  boolean     bool                                             PLAIN (V2 pages may come out RLE: then 1, behind the hybrid decoder)
  strings     string: lengths 0, 1, 63, 64, 65 and about 300 among short ones   PLAIN, DELTA_LENGTH_BYTE_ARRAY
  delta       int64                                            DELTA_BINARY_PACKED       8, behind the delta decoder
The encoding is read from every page's header and asserted, not assumed.  Per file <version>_<column>_<encoding>_<part>.bin
and .json (a column's pages go to as many parts as keep every file under LIMIT bytes): every data page's
definition-level stream and, right behind it, its values section as they lie in the file, and what the page's rows hold
-- pinned to the table pyarrow was given, not to any decoder: a level of 1 where the row is not null, the validity
bitmap, and the rows' values (zero bytes where the row is null), their bits, or the Arrow offsets and the bytes."""
import decimal
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

ROWS = 1500
LIMIT = 27000                # no file larger than the largest of ../parquet_dict
PLAIN, RLE, DELTA_BINARY_PACKED, DELTA_LENGTH_BYTE_ARRAY, BYTE_STREAM_SPLIT = 0, 3, 5, 6, 9
JULIAN_EPOCH = 2440588


def int96(ns):
    """a timestamp of `ns` nanoseconds since 1970 as Parquet's INT96"""
    day, rest = divmod(ns, 86400 * 10 ** 9)
    return struct.pack("<qI", rest, JULIAN_EPOCH + day)


def flba(unscaled, n):
    return unscaled.to_bytes(n, "big", signed=True)


def columns():
    """[(column, arrow type, the rows' values, pyarrow's encoding, the fixture's encoding, the Parquet encoding of its
    pages, value bytes or 0, value -> its bytes)]"""
    rng = np.random.default_rng(30)
    ints = [int(v) for v in rng.integers(-2 ** 31, 2 ** 31, ROWS)]
    longs = [int(v) for v in rng.integers(-2 ** 63, 2 ** 63, ROWS)]
    floats = [float(np.float32(v)) for v in rng.normal(0, 1000, ROWS)]
    doubles = [float(v) for v in rng.normal(0, 1e9, ROWS)]
    stamps = [int(v) for v in rng.integers(0, 2 * 10 ** 18, ROWS)]
    small = [int(v) for v in rng.integers(-10 ** 11 + 1, 10 ** 11, ROWS)]
    wide = [int(v) * 10 ** 19 + int(u) for v, u in zip(rng.integers(-10 ** 18, 10 ** 18, ROWS), rng.integers(0, 10 ** 18, ROWS))]
    flags = [bool(v) for v in rng.integers(0, 2, ROWS)]
    walk = [int(v) for v in np.cumsum(rng.integers(-1000, 100000, ROWS))]
    letters = "abcdefghijklmnopqrstuvwxyz"
    word = lambda n: "".join(letters[int(c)] for c in rng.integers(0, 26, n))
    texts = [word(int(n)) for n in rng.integers(0, 9, ROWS)]
    for k, t in enumerate(["", word(1), word(63), word(64), word(65), word(301)]):   # (twice each, and not in a null row)
        texts[1 + k] = texts[1100 + k] = t
    i32, i64 = (lambda v: struct.pack("<i", v)), (lambda v: struct.pack("<q", v))
    f32, f64 = (lambda v: struct.pack("<f", v)), (lambda v: struct.pack("<d", v))
    return [("int32", pa.int32(), ints, "PLAIN", "plain", PLAIN, 4, i32),
            ("int64", pa.int64(), longs, "PLAIN", "plain", PLAIN, 8, i64),
            ("float", pa.float32(), floats, "PLAIN", "plain", PLAIN, 4, f32),
            ("float", pa.float32(), floats, "BYTE_STREAM_SPLIT", "split", BYTE_STREAM_SPLIT, 4, f32),
            ("double", pa.float64(), doubles, "PLAIN", "plain", PLAIN, 8, f64),
            ("double", pa.float64(), doubles, "BYTE_STREAM_SPLIT", "split", BYTE_STREAM_SPLIT, 8, f64),
            ("int96", pa.timestamp("ns"), stamps, "PLAIN", "plain", PLAIN, 12, int96),
            ("decimal5", pa.decimal128(11, 2), small, "PLAIN", "plain", PLAIN, 5, lambda v: flba(v, 5)),
            ("decimal16", pa.decimal128(38, 4), wide, "PLAIN", "plain", PLAIN, 16, lambda v: flba(v, 16)),
            ("boolean", pa.bool_(), flags, "PLAIN", "boolean", PLAIN, 0, None),
            ("strings", pa.string(), texts, "PLAIN", "prefixed", PLAIN, 0, lambda v: v.encode()),
            ("strings", pa.string(), texts, "DELTA_LENGTH_BYTE_ARRAY", "packed", DELTA_LENGTH_BYTE_ARRAY, 0, lambda v: v.encode()),
            ("delta", pa.int64(), walk, "DELTA_BINARY_PACKED", "delta", DELTA_BINARY_PACKED, 8, i64)]


def arrow_value(kind, v):
    if pa.types.is_decimal(kind):
        return decimal.Decimal(v).scaleb(-kind.scale)
    return v


def main():
    for version in ("1.0", "2.0"):
        for column, kind, values, asked, encoding, parquet_encoding, value_bytes, encode in columns():
            rows = [None if i % 7 == 0 or 600 <= i < 1000 else v for i, v in enumerate(values)]
            sink = io.BytesIO()
            with decimal.localcontext() as ctx:
                ctx.prec = 60
                array = pa.array([None if v is None else arrow_value(kind, v) for v in rows], kind)
            pq.write_table(pa.table({"c": array}), sink, use_dictionary=False, column_encoding={"c": asked}, compression="none",
                           data_page_version=version, data_page_size=256, write_batch_size=64, max_rows_per_page=100,
                           use_deprecated_int96_timestamps=column == "int96", store_decimal_as_integer=False)
            data = sink.getvalue()
            col = pq.ParquetFile(io.BytesIO(data)).metadata.row_group(0).column(0)
            assert not col.has_dictionary_page
            start = col.data_page_offset
            chunk = data[start:start + col.total_compressed_size]
            pages = P.walk(chunk, P.UNCOMPRESSED)
            # a V2 boolean page may come out RLE: then the fixture is one of 1-byte values behind decode_parquet_hybrid
            mine, width = encoding, value_bytes
            if column == "boolean" and all(p["encoding"] == RLE for p in pages):
                mine, parquet_encoding, width = "rle_boolean", RLE, 1
            parts, blob, listed, row = [], bytearray(), [], 0

            def put(b):
                at = len(blob)
                blob.extend(b)
                return [at, len(b)]

            for p in pages:
                assert p["encoding"] == parquet_encoding, ("a page of another encoding", column, asked, p["encoding"])
                body = chunk[p["body_offset"]:p["body_offset"] + p["compressed_page_size"]]
                if p["kind"] == P.DATA_PAGE_V2:
                    assert p["rep_levels_bytes"] == 0
                    levels = p["def_levels_bytes"]
                else:
                    assert p["kind"] == P.DATA_PAGE
                    levels = 4 + struct.unpack_from("<I", body)[0]
                rows_here = rows[row:row + p["num_values"]]
                row += p["num_values"]
                there = [v for v in rows_here if v is not None]
                bits = sum((v is not None) << i for i, v in enumerate(rows_here))
                entry = dict(num_values=p["num_values"], non_null=len(there), level_stream=put(body[:levels]), values=put(body[levels:]),
                             expected_levels=put(bytes(v is not None for v in rows_here)),
                             expected_validity=put(bits.to_bytes((len(rows_here) + 7) // 8, "little")))
                if mine == "boolean":
                    set_bits = sum(bool(v) << i for i, v in enumerate(rows_here))
                    entry["expected_bits"] = put(set_bits.to_bytes((len(rows_here) + 7) // 8, "little"))
                elif mine == "rle_boolean":
                    entry["expected_values"] = put(bytes(bool(v) for v in rows_here))
                elif width:
                    assert all(len(encode(v)) == width for v in there)
                    entry["expected_values"] = put(b"".join(bytes(width) if v is None else encode(v) for v in rows_here))
                else:
                    offsets = [0]
                    for v in rows_here:
                        offsets.append(offsets[-1] + (0 if v is None else len(encode(v))))
                    entry["expected_offsets"] = put(struct.pack("<%di" % len(offsets), *offsets))
                    entry["expected_bytes"] = put(b"".join(encode(v) for v in there))
                listed.append(entry)
                if len(blob) > LIMIT - 3000:
                    parts.append((bytes(blob), listed))
                    blob, listed = bytearray(), []
            if listed:
                parts.append((bytes(blob), listed))
            every = [e for _, part in parts for e in part]
            assert row == ROWS and len(every) >= 4, (column, len(every))
            assert any(e["non_null"] == 0 and e["num_values"] for e in every), "no page is wholly null"
            for k, (part, entries) in enumerate(parts):
                name = "v%s_%s_%s_%d" % (version[0], column, mine, k)
                with open(os.path.join(HERE, name + ".bin"), "wb") as f:
                    f.write(part)
                with open(os.path.join(HERE, name + ".json"), "w") as f:
                    json.dump(dict(pyarrow=pa.__version__, data_page_version=version, column=column, encoding=mine, value_bytes=width,
                                   pages=entries), f, indent=None, separators=(",", ":"))
                    f.write("\n")
                size = os.path.getsize(os.path.join(HERE, name + ".json"))
                assert len(part) <= LIMIT and size <= LIMIT, (name, len(part), size)
                print(name, len(part), "bytes,", len(entries), "pages")


if __name__ == "__main__":
    main()
