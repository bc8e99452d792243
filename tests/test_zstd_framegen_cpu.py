"""The planned-frame writer (tests/zstd_framegen.py) against libzstd on the CPU: every legal plan is accepted with
the planned bytes, every illegal plan is refused, and the inspector shows every planned form in at least one frame
libzstd accepts -- the condition that keeps a silently dropped plan from passing."""
import zstd_fixtures as F
import zstd_framegen as G


def test_libzstd_loads():
    z = G.libzstd()
    assert z is not None, "libzstd.so.1 does not load: it is the arbiter of the Zstandard tests"
    assert z.ZSTD_versionNumber() >= 10400


def test_every_legal_plan_is_accepted_with_its_bytes():
    for name, chunk, content, _ in G.legal_plans():
        assert G.arbiter(chunk, len(content)) == content, name
        assert G.arbiter(chunk, len(content) + 1000) == content, name
        if content:
            assert G.arbiter(chunk, len(content) - 1) is None, name


def test_every_form_occurs_in_a_frame_libzstd_accepts():
    planned = set()
    for name, chunk, content, forms in G.legal_plans():
        if G.arbiter(chunk, len(content)) == content:
            planned |= forms | G.inspect(chunk)
    assert G.LEGAL_FORMS_PLANNED - planned == set()
    made = set()
    for name, chunk, content in F.load()[0]:
        if G.arbiter(chunk, len(content)) == content:
            made |= G.inspect(chunk)
    assert G.LEGAL_FORMS_FROM_LIBZSTD - made == set()


def test_every_illegal_plan_is_refused():
    plans = G.illegal_plans()
    assert len({n for n, _ in plans}) == len(plans) >= 25
    for name, chunk in plans:
        assert G.arbiter(chunk, 1 << 17) is None, name


def test_documented_differences_are_accepted_by_libzstd():
    for name, chunk in G.documented_differences():
        assert G.arbiter(chunk, 1 << 17) is not None, name


def test_xxh64_of_the_writer_is_libzstd_s():
    # a frame with a checksum is accepted only with the right one
    fr, content, _ = G.frame([("raw", b"checksummed content " * 9)], checksum=True)
    assert G.arbiter(fr, len(content)) == content
    assert G.arbiter(fr[:-4] + bytes([fr[-4] ^ 1]) + fr[-3:], len(content)) is None
