"""bench.py --dump-outputs on CPU: what dump_outputs writes for a job's last step -- the per-chunk sizes and
statuses, and a seeded sample of chunks whose bytes past their sizes are zero -- and that two runs pick the
same sample."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _fake_job(n, comp_stride, out_stride, seed):
    """The buffers of bench.CodecJob that a caller of the timed path receives, on the CPU: slots filled with
    garbage beyond each chunk's size, as the device buffers are."""
    g = torch.Generator().manual_seed(seed)
    comp = SimpleNamespace(data=torch.randint(0, 256, (n * comp_stride,), dtype=torch.uint8, generator=g),
                           sizes=torch.randint(0, comp_stride + 1, (n,), dtype=torch.int64, generator=g),
                           stride=comp_stride)
    out = SimpleNamespace(data=torch.randint(0, 256, (n * out_stride,), dtype=torch.uint8, generator=g),
                          sizes=None, stride=out_stride)
    actual = torch.randint(0, out_stride + 1, (n,), dtype=torch.int64, generator=g)
    return SimpleNamespace(n=n, comp=comp, out=out, actual=actual,
                           statuses=torch.zeros(n, dtype=torch.int32))


def test_dump_outputs_writes_sizes_and_a_seeded_sample(tmp_path):
    import bench
    n = 300
    job = _fake_job(n, 96, 64, 1)
    bench.dump_outputs(job, str(tmp_path / "a"))
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert set(got) == {"sample_chunks", "compressed_sizes", "compressed_sample", "decompressed_sizes",
                        "decompressed_sample", "statuses"}
    assert all(a.dtype == np.float32 for a in got.values())
    assert np.array_equal(got["compressed_sizes"], job.comp.sizes.numpy())
    assert np.array_equal(got["decompressed_sizes"], job.actual.numpy())
    assert np.array_equal(got["statuses"], job.statuses.numpy())
    pick = got["sample_chunks"].astype(np.int64)
    assert len(pick) == bench.DUMP_SAMPLE_CHUNKS and len(set(pick.tolist())) == len(pick)
    assert got["compressed_sample"].shape == (len(pick), 96) and got["decompressed_sample"].shape == (len(pick), 64)
    for batch, sizes, rows in ((job.comp, job.comp.sizes, got["compressed_sample"]),
                               (job.out, job.actual, got["decompressed_sample"])):
        host = batch.data.numpy().reshape(n, batch.stride)
        for r, i in enumerate(pick):
            k = int(sizes[i])
            assert np.array_equal(rows[r, :k], host[i, :k]) and not rows[r, k:].any()

    # another run of the same workload: the same chunks are sampled, so the files compare one for one
    bench.dump_outputs(_fake_job(n, 96, 64, 2), str(tmp_path / "b"))
    assert np.array_equal(np.load(tmp_path / "b" / "sample_chunks.npy"), got["sample_chunks"])


def test_dump_outputs_of_a_batch_smaller_than_the_sample(tmp_path):
    import bench
    bench.dump_outputs(_fake_job(5, 32, 16, 3), str(tmp_path))
    assert np.array_equal(np.load(tmp_path / "sample_chunks.npy"), np.arange(5, dtype=np.float32))
    assert np.load(tmp_path / "compressed_sample.npy").shape == (5, 32)
