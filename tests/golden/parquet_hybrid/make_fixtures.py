"""Writes the fixtures of this directory; needed only to make them again (it needs pyarrow; the tests read the files).

pyarrow writes a nullable int64 column of 5000 rows, dictionary-encoded and uncompressed, under data_page_version "1.0"
and "2.0", its keys drawn from 1, 2, 3, 37, 300 and 5000 values: rows 1000 to 1399 hold one key, every seventh row and
rows 2000 to 2299 are null.  Per file <version>_c<cardinality>.bin and .json: every data page's definition-level stream
and dictionary-index stream as they lie in the file, and what they hold -- pinned to the table pyarrow was given (a
level of 1 where the row is not null; the place of the row's key in the dictionary page, whose PLAIN int64 values are
read here), not to any decoder of hybrid streams."""
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


def column(cardinality):
    rng = np.random.default_rng(cardinality)
    keys = [int(k) * 1000003 + 17 for k in rng.integers(0, cardinality, ROWS)]
    for i in range(1000, 1400):
        keys[i] = keys[1000]
    return [None if i % 7 == 0 or 2000 <= i < 2300 else keys[i] for i in range(ROWS)]


def main():
    for version in ("1.0", "2.0"):
        for cardinality in (1, 2, 3, 37, 300, 5000):
            rows = column(cardinality)
            sink = io.BytesIO()
            pq.write_table(pa.table({"c": pa.array(rows, pa.int64())}), sink, use_dictionary=True, compression="none",
                           data_page_version=version, data_page_size=1024, write_batch_size=128)
            data = sink.getvalue()
            col = pq.ParquetFile(io.BytesIO(data)).metadata.row_group(0).column(0)
            assert col.has_dictionary_page
            chunk = data[col.dictionary_page_offset:col.dictionary_page_offset + col.total_compressed_size]
            pages = P.walk(chunk, P.UNCOMPRESSED)
            assert pages[0]["kind"] == P.DICTIONARY_PAGE and pages[0]["encoding"] in (0, 2)
            body = chunk[pages[0]["body_offset"]:pages[0]["body_offset"] + pages[0]["compressed_page_size"]]
            place = {key: k for k, key in enumerate(struct.unpack("<%dq" % pages[0]["num_values"], body))}
            blob, listed, row = bytearray(), [], 0

            def put(b):
                at = len(blob)
                blob.extend(b)
                return [at, len(b)]

            for p in pages[1:]:
                assert p["encoding"] in (2, 8), "a page fell back to PLAIN"
                body = chunk[p["body_offset"]:p["body_offset"] + p["compressed_page_size"]]
                if p["kind"] == P.DATA_PAGE_V2:
                    assert p["rep_levels_bytes"] == 0
                    levels = p["def_levels_bytes"]
                else:
                    assert p["kind"] == P.DATA_PAGE
                    levels = 4 + struct.unpack_from("<I", body)[0]
                mine = rows[row:row + p["num_values"]]
                row += p["num_values"]
                there = [place[key] for key in mine if key is not None]
                listed.append(dict(num_values=p["num_values"], non_null=len(there), index_bit_width=body[levels],
                                   level_stream=put(body[:levels]), index_stream=put(body[levels:]),
                                   expected_levels=put(bytes(key is not None for key in mine)),
                                   expected_indices=put(struct.pack("<%dI" % len(there), *there))))
            assert row == ROWS and len(listed) > 1 and len(blob) < 65536
            name = "v%s_c%d" % (version[0], cardinality)
            with open(os.path.join(HERE, name + ".bin"), "wb") as f:
                f.write(blob)
            with open(os.path.join(HERE, name + ".json"), "w") as f:
                json.dump(dict(pyarrow=pa.__version__, data_page_version=version, cardinality=cardinality,
                               dictionary_entries=len(place), pages=listed), f, indent=1)
                f.write("\n")
            print(name, len(blob), "bytes,", len(listed), "pages, widths", sorted({p["index_bit_width"] for p in listed}))


if __name__ == "__main__":
    main()
