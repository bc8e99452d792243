"""Writes the fixtures of this directory; needed only to make them again (it needs pyarrow; the tests read the files).

pyarrow writes nullable columns of 1500 rows, dictionary-encoded and uncompressed, under data_page_version "1.0" and
"2.0": every seventh row and rows 600 to 999 are null, so one page at least is wholly null; data_page_size is small, so a
chunk has several data pages on its one dictionary page.
  int32      int32                              4-byte entries
  int64      int64                              8
  float      float32                            4
  double     float64                            8
  int96      timestamp[ns], use_deprecated_int96_timestamps: nanoseconds of the day, then the Julian day   12
  decimal5   decimal128(11, 2), FIXED_LEN_BYTE_ARRAY of 5 bytes, big-endian two's complement               5
  decimal16  decimal128(38, 4), FIXED_LEN_BYTE_ARRAY of 16 bytes                                           16
  strings    string: empty strings, and entries of 1, 63, 64, 65 and about 300 bytes among short ones
Per file <version>_<column>.bin and .json: the dictionary page's body, every data page's definition-level stream and
index stream (everything of the page behind the levels: a width byte, then the runs) as they lie in the file, and what
the page's rows hold -- pinned to the table pyarrow was given, not to any decoder: a level of 1 where the row is not
null, the validity bitmap, the rows' entries (zero bytes where the row is null), or the Arrow offsets and the bytes."""
import datetime
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
PLAIN_DICTIONARY, RLE_DICTIONARY = 2, 8
EPOCH = datetime.datetime(1970, 1, 1)
JULIAN_EPOCH = 2440588


def int96(ns):
    """a timestamp of `ns` nanoseconds since 1970 as Parquet's INT96"""
    day, rest = divmod(ns, 86400 * 10 ** 9)
    return struct.pack("<qI", rest, JULIAN_EPOCH + day)


def flba(unscaled, n):
    return unscaled.to_bytes(n, "big", signed=True)


def columns():
    """name -> (arrow type, the rows' values, their entry bytes or None for strings, value -> the entry's bytes)"""
    rng = np.random.default_rng(29)
    pick = lambda pool: [pool[int(i)] for i in rng.integers(0, len(pool), ROWS)]
    ints = [int(v) for v in rng.integers(-2 ** 31, 2 ** 31, 200)]
    longs = [int(v) for v in rng.integers(-2 ** 63, 2 ** 63, 150)]
    floats = [float(np.float32(v)) for v in rng.normal(0, 1000, 100)]
    doubles = [float(v) for v in rng.normal(0, 1e9, 120)]
    stamps = [int(v) for v in rng.integers(0, 2 * 10 ** 18, 90)]
    small = [int(v) for v in rng.integers(-10 ** 11 + 1, 10 ** 11, 60)]
    wide = [int(v) * 10 ** 19 + int(u) for v, u in zip(rng.integers(-10 ** 18, 10 ** 18, 70), rng.integers(0, 10 ** 18, 70))]
    letters = "abcdefghijklmnopqrstuvwxyz"
    word = lambda n: "".join(letters[int(c)] for c in rng.integers(0, 26, n))
    texts = [word(int(n)) for n in rng.integers(0, 9, 40)] + ["", word(1), word(63), word(64), word(65), word(301)]
    rare = pick(texts[:40])
    for k, t in enumerate(texts[40:]):       # (each of the others twice, and not in a null row)
        rare[1 + k] = rare[1100 + k] = t
    return {"int32": (pa.int32(), pick(ints), 4, lambda v: struct.pack("<i", v)),
            "int64": (pa.int64(), pick(longs), 8, lambda v: struct.pack("<q", v)),
            "float": (pa.float32(), pick(floats), 4, lambda v: struct.pack("<f", v)),
            "double": (pa.float64(), pick(doubles), 8, lambda v: struct.pack("<d", v)),
            "int96": (pa.timestamp("ns"), pick(stamps), 12, int96),
            "decimal5": (pa.decimal128(11, 2), pick(small), 5, lambda v: flba(v, 5)),
            "decimal16": (pa.decimal128(38, 4), pick(wide), 16, lambda v: flba(v, 16)),
            "strings": (pa.string(), rare, None, lambda v: v.encode())}


def arrow_value(kind, v):
    if pa.types.is_decimal(kind):
        return decimal.Decimal(v).scaleb(-kind.scale)
    return v


def main():
    for version in ("1.0", "2.0"):
        for column, (kind, values, element, encode) in columns().items():
            rows = [None if i % 7 == 0 or 600 <= i < 1000 else v for i, v in enumerate(values)]
            sink = io.BytesIO()
            with decimal.localcontext() as ctx:
                ctx.prec = 60
                array = pa.array([None if v is None else arrow_value(kind, v) for v in rows], kind)
            pq.write_table(pa.table({"c": array}), sink, use_dictionary=True, compression="none", data_page_version=version,
                           data_page_size=256, write_batch_size=64, use_deprecated_int96_timestamps=column == "int96",
                           store_decimal_as_integer=False)
            data = sink.getvalue()
            col = pq.ParquetFile(io.BytesIO(data)).metadata.row_group(0).column(0)
            assert col.has_dictionary_page
            start = col.dictionary_page_offset
            chunk = data[start:start + col.total_compressed_size]
            pages = P.walk(chunk, P.UNCOMPRESSED)
            blob, listed, row = bytearray(), [], 0

            def put(b):
                at = len(blob)
                blob.extend(b)
                return [at, len(b)]

            assert pages[0]["kind"] == P.DICTIONARY_PAGE and all(p["kind"] != P.DICTIONARY_PAGE for p in pages[1:])
            d = pages[0]
            dictionary = put(chunk[d["body_offset"]:d["body_offset"] + d["compressed_page_size"]])
            for p in pages[1:]:
                assert p["encoding"] in (PLAIN_DICTIONARY, RLE_DICTIONARY), "a page fell back"
                body = chunk[p["body_offset"]:p["body_offset"] + p["compressed_page_size"]]
                if p["kind"] == P.DATA_PAGE_V2:
                    assert p["rep_levels_bytes"] == 0
                    levels = p["def_levels_bytes"]
                else:
                    assert p["kind"] == P.DATA_PAGE
                    levels = 4 + struct.unpack_from("<I", body)[0]
                mine = rows[row:row + p["num_values"]]
                row += p["num_values"]
                there = [encode(v) for v in mine if v is not None]
                bits = sum((v is not None) << i for i, v in enumerate(mine))
                entry = dict(num_values=p["num_values"], non_null=len(there), level_stream=put(body[:levels]),
                             index_stream=put(body[levels:]), expected_levels=put(bytes(v is not None for v in mine)),
                             expected_validity=put(bits.to_bytes((len(mine) + 7) // 8, "little")))
                if element:
                    assert all(len(e) == element for e in there)
                    entry["expected_values"] = put(b"".join(bytes(element) if v is None else encode(v) for v in mine))
                else:
                    offsets = [0]
                    for v in mine:
                        offsets.append(offsets[-1] + (0 if v is None else len(encode(v))))
                    entry["expected_offsets"] = put(struct.pack("<%di" % len(offsets), *offsets))
                    entry["expected_bytes"] = put(b"".join(there))
                listed.append(entry)
            assert row == ROWS and len(listed) >= 4 and len(blob) < 65536, (column, len(listed), len(blob))
            assert any(p["non_null"] == 0 and p["num_values"] for p in listed), "no page is wholly null"
            name = "v%s_%s" % (version[0], column)
            with open(os.path.join(HERE, name + ".bin"), "wb") as f:
                f.write(blob)
            with open(os.path.join(HERE, name + ".json"), "w") as f:
                json.dump(dict(pyarrow=pa.__version__, data_page_version=version, column=column, entry_bytes=element or 0,
                               dictionary=dictionary, dictionary_entries=d["num_values"], pages=listed), f, indent=1)
                f.write("\n")
            print(name, len(blob), "bytes,", len(listed), "pages,", d["num_values"], "entries of", dictionary[1], "bytes")


if __name__ == "__main__":
    main()
