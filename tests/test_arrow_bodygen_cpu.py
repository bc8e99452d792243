"""The Arrow IPC fixtures of tests/golden/arrow_ipc/ (tests/arrow_bodygen.py wrote them; tests/test_lz4_frames_gpu.py
reads them through decompress_frames): every item of the committed bodies is held to liblz4's LZ4F_decompress through
ctypes, as the frame tests hold theirs, and -- where pyarrow imports -- to pyarrow's own codec and to what the
generator makes today."""
import hashlib
import struct

import pytest

import arrow_bodygen as A
import lz4_framegen as G


@pytest.fixture(scope="module", params=A.FIXTURES)
def fixture(request):
    return (request.param,) + A.load(request.param)


def test_manifest_is_sound(fixture):
    name, body, items = fixture
    assert len(body) < 64 << 10, "a committed fixture stays small"
    end = 0
    for it in items:
        assert it["offset"] == end and it["offset"] % 8 == 0, "items stand one behind the other, padded to 8"
        end = it["offset"] + it["length"] + (-it["length"] % 8)
        assert body[it["offset"] + it["length"]:end] == bytes(end - it["offset"] - it["length"])
    assert end == len(body), "the items cover the body"
    blocks = []
    for it in items:
        if it["length"] == 0:
            assert it["decoded_size"] == 0
            continue
        p, = struct.unpack_from("<q", body, it["offset"])
        assert p == (-1 if it["stored"] else it["decoded_size"])
        if not it["stored"]:
            assert A.frame_end(body, it["offset"] + 8) == it["offset"] + it["length"], "one frame, nothing behind it"
            flg = body[it["offset"] + 12]
            blocks.append((not flg & 0x20, None))
    # what the GPU tests rely on: linked frames of several blocks and a frame of one independent block
    assert any(linked for linked, _ in blocks) and any(not linked for linked, _ in blocks)
    if name == "codec":
        assert [it["stored"] for it in items].count(True) == 1 and [it["length"] for it in items].count(0) == 1
    else:
        assert walked(body) == [(it["offset"], it["length"], it["decoded_size"]) for it in items]


def walked(body):
    return A.walk(body)


def test_items_decode_with_liblz4(fixture):
    _, body, items = fixture
    L = G.load_lz4f()
    if L is None:
        pytest.skip("liblz4.so.1 absent")
    for it in items:
        piece = body[it["offset"]:it["offset"] + it["length"]]
        if it["length"] == 0:
            data = b""
        elif it["stored"]:
            data = piece[8:]
        else:
            ok, data = G.lz4f_decompress(L, piece[8:])
            assert ok
        assert len(data) == it["decoded_size"] and hashlib.sha256(data).hexdigest() == it["sha256"], it


def test_items_decode_with_pyarrow(fixture):
    pa = pytest.importorskip("pyarrow")
    _, body, items = fixture
    codec = pa.Codec("lz4")
    for it in items:
        if it["length"] == 0 or it["stored"]:
            continue
        data = codec.decompress(body[it["offset"] + 8:it["offset"] + it["length"]], it["decoded_size"]).to_pybytes()
        assert hashlib.sha256(data).hexdigest() == it["sha256"], it


def test_generator_decodes_to_the_fixture(fixture):
    """what the generator makes with the pyarrow at hand decodes, buffer for buffer, to what the fixture holds (the
    compressed bytes may differ from one liblz4 to the next; the buffers may not)"""
    pytest.importorskip("pyarrow")
    name, _, items = fixture
    _, fresh = A.record_batch_body() if name == "record_batch" else A.codec_body()
    assert [(it["decoded_size"], it["sha256"], it["stored"]) for it in fresh] \
        == [(it["decoded_size"], it["sha256"], it["stored"]) for it in items]
