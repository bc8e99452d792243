"""The damaged Cascaded corpus of tests/test_decode_containment_gpu.py through the CPU oracle alone: an oracle that
misreads a hostile stream shows up here, on a machine without a GPU, before it can take a GPU run down with it.
Every status is 0 or 12, the reported size is 0 on failure and the declared element count x element size on
success, and the undamaged streams round-trip."""
import decode_guard as G


def test_damaged_cascaded_streams_through_the_oracle(oracle):
    corpus = G.cascaded_corpus(oracle)
    assert sum(good for *_, good in corpus) == 8 * len(G.CASCADED_OPTS) * 3
    seen = {0: 0, 12: 0}
    for k, (s, src, t, good) in enumerate(corpus):
        for cap in sorted(set(G.capacity_kinds(len(src), G.CASCADED_SIZE[t]))):
            st, out = oracle.cascaded_decompress(s, cap)
            assert st in (0, 12), (k, cap, st)
            seen[st] += 1
            if st != 0:
                assert out == b"", (k, cap)
                continue
            es = G.CASCADED_SIZE[s[3]]
            declared = int.from_bytes(s[4:8], "little")
            assert len(out) == declared // es * es <= cap, (k, cap)
            if good:
                assert out == src, (k, cap)
        if good:
            assert oracle.cascaded_decompress(s, len(src)) == (0, src), k
    assert seen[0] and seen[12]
