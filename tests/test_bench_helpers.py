"""CPU tests for bench.py's input generators: the signer-key sums gate the
bench's correctness check, so their exact-arithmetic trick (8-bit chunk
float32 sgemm, sums < 2^24) must itself be pinned."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402


def test_signer_sums_exact():
    import numpy as np
    from oracle import pyref as pr
    rng = np.random.default_rng(77)
    n = 700
    sk_ints = [pr.synth_sk(i) for i in range(n)]
    chunks8 = np.array([[(s >> (8 * j)) & 0xFF for j in range(32)]
                        for s in sk_ints], dtype=np.float32)
    bits = bench._rand_bits(rng, 5, n, 0.5)
    sums = bench._signer_sums(bits, chunks8, pr.R)
    for b in range(5):
        want = sum(sk_ints[i] for i in np.nonzero(bits[b])[0]) % pr.R
        assert sums[b] == want


def test_dump_outputs_float32_npy(tmp_path):
    import numpy as np
    d = tmp_path / "sub" / "dump"          # created on demand
    bench.dump_outputs(str(d), {"verify_results": [1, 0, 1],
                                "rows": bench._bytes_rows(bytes(range(12)), 4)})
    v = np.load(d / "verify_results.npy")
    assert v.dtype == np.float32 and v.tolist() == [1.0, 0.0, 1.0]
    r = np.load(d / "rows.npy")
    assert r.dtype == np.float32 and r.shape == (3, 4) and r[2, 3] == 11.0


def test_dump_outputs_caps_total_size_with_fixed_sample(tmp_path, monkeypatch):
    import numpy as np
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 4 * 200)   # 100 elements each
    big = np.arange(1000)
    small = np.arange(50)
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.shape == (100,) and (a == b).all()       # same sample every run
    assert (np.diff(a) > 0).all()                      # drawn without repeats
    assert (np.load(tmp_path / "a" / "small.npy") == small).all()
    written = sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in ("big.npy", "small.npy"))
    assert written <= 4 * 200                          # payload within the cap


def test_rank_name():
    assert bench._rank_name("verify_results", 0, 1) == "verify_results"
    assert bench._rank_name("verify_results", 3, 8) == "verify_results_rank3"


def test_rand_bits_deterministic_and_dense():
    import numpy as np
    a = bench._rand_bits(np.random.default_rng(5), 4, 1000, 0.9)
    b = bench._rand_bits(np.random.default_rng(5), 4, 1000, 0.9)
    assert (a == b).all()
    density = a.mean()
    assert 0.85 < density < 0.95
