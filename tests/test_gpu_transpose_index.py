"""tcsc_gpu_transpose_index: the TCSC arrays of W[:, c0:c1]^T from those of W, on
the device, bit for bit what the reference's tcsc_from_dense (tcsc.c:6-66) gives
for the dense transposed slice -- ascending inside every output column whatever
order the integer atomics of the build land in."""
import numpy as np
import pytest

import tcsc_amd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    tcsc_amd.build()
    tcsc_amd.require_gpu()
    return torch


def dev_i32(torch, a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    t = torch.empty(max(a.size, 1), dtype=torch.int32, device="cuda:0")
    if a.size:
        t[:a.size] = torch.from_numpy(a)
    return t


def transpose_on_gpu(torch, K, N, arrays, c0, c1):
    """(t_csp, t_csn, t_rip, t_rin) as numpy, from W's four host arrays."""
    csp, csn, rip, rin = arrays
    n_pos, n_neg = int(csp[c1] - csp[c0]), int(csn[c1] - csn[c0])
    d = [dev_i32(torch, a) for a in arrays]
    # sentinels: every offset must be written, nothing past the counted sizes
    t_csp = torch.full((K + 1,), -7, dtype=torch.int32, device="cuda:0")
    t_csn = torch.full((K + 1,), -7, dtype=torch.int32, device="cuda:0")
    t_rip = torch.full((n_pos + 3,), -7, dtype=torch.int32, device="cuda:0")
    t_rin = torch.full((n_neg + 3,), -7, dtype=torch.int32, device="cuda:0")
    tcsc_amd.gpu_transpose_index(K, N, d[0], d[1], d[2], d[3], c0, c1, t_csp, t_csn, t_rip, t_rin,
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (t_rip[n_pos:] == -7).all() and (t_rin[n_neg:] == -7).all(), "wrote past the counted entries"
    return t_csp.cpu().numpy(), t_csn.cpu().numpy(), t_rip[:n_pos].cpu().numpy(), t_rin[:n_neg].cpu().numpy()


def check_against_oracle(torch, oracle, Wd, c0, c1, arrays=None):
    K, N = Wd.shape
    arrays = oracle.tcsc_from_dense(Wd).arrays() if arrays is None else arrays
    got = transpose_on_gpu(torch, K, N, arrays, c0, c1)
    want = oracle.tcsc_from_dense(np.ascontiguousarray(Wd[:, c0:c1].T)).arrays()
    for name, g, w in zip(("t_col_start_pos", "t_col_start_neg", "t_row_index_pos", "t_row_index_neg"), got, want):
        assert g.dtype == np.int32 and g.shape == w.shape, name
        np.testing.assert_array_equal(g, w, err_msg=name)
    return got


SHAPES = [(1, 1, 1.0), (7, 5, 0.5), (300, 1000, 0.05), (1000, 300, 0.05), (4097, 130, 0.3), (64, 3000, 1.0)]


@pytest.mark.parametrize("K,N,density", SHAPES)
def test_transpose_matches_tcsc_from_dense_of_the_transpose(torch_gpu, oracle, K, N, density):
    Wd = oracle.ternary((K, N), density, 4000 + K + N)
    ranges = [(0, N)] + ([(37, 400)] if N >= 400 else [])
    for c0, c1 in ranges:
        check_against_oracle(torch_gpu, oracle, Wd, c0, c1)


def test_only_positive_entries(torch_gpu, oracle):
    Wd = np.abs(oracle.ternary((50, 70), 0.2, 4100))
    got = check_against_oracle(torch_gpu, oracle, Wd, 0, 70)
    assert got[3].size == 0 and not got[1].any()
    check_against_oracle(torch_gpu, oracle, Wd, 11, 64)


def test_empty_border_rows_and_columns(torch_gpu, oracle):
    Wd = oracle.ternary((40, 90), 0.3, 4101)
    Wd[0, :] = 0
    Wd[-1, :] = 0
    Wd[:, 0] = 0
    Wd[:, -1] = 0
    got = check_against_oracle(torch_gpu, oracle, Wd, 0, 90)
    assert got[0][1] == 0 and got[0][-1] == got[0][-2]  # output columns 0 and K-1 are empty
    check_against_oracle(torch_gpu, oracle, Wd, 0, 1)  # a range holding only the empty column


def test_zero_rows(torch_gpu, oracle):
    Wd = np.zeros((0, 5), np.float32)
    got = check_against_oracle(torch_gpu, oracle, Wd, 0, 5)
    assert [g.tolist() for g in got] == [[0], [0], [], []]


def test_empty_range_writes_zero_offsets(torch_gpu, oracle):
    Wd = oracle.ternary((20, 9), 0.5, 4102)
    got = check_against_oracle(torch_gpu, oracle, Wd, 3, 3)
    assert not got[0].any() and not got[1].any() and got[0].size == 21


def test_unsorted_input_column_gives_the_same_output(torch_gpu, oracle):
    Wd = oracle.ternary((60, 40), 0.4, 4103)
    csp, csn, rip, rin = oracle.tcsc_from_dense(Wd).arrays()
    j = int(np.argmax(np.diff(csp)))
    assert csp[j + 1] - csp[j] >= 3
    rip = rip.copy()
    rip[csp[j]:csp[j + 1]] = rip[csp[j]:csp[j + 1]][::-1]  # descending
    check_against_oracle(torch_gpu, oracle, Wd, 0, 40, (csp, csn, rip, rin))
    check_against_oracle(torch_gpu, oracle, Wd, max(j - 2, 0), min(j + 3, 40), (csp, csn, rip, rin))


def test_row_index_out_of_range_is_an_argument_error(torch_gpu, oracle):
    K, N = 30, 20
    Wd = oracle.ternary((K, N), 0.4, 4104)
    csp, csn, rip, rin = oracle.tcsc_from_dense(Wd).arrays()
    rin = rin.copy()
    rin[rin.size // 2] = K
    with pytest.raises(tcsc_amd.TcscError, match=r"status 1\)"):
        transpose_on_gpu(torch_gpu, K, N, (csp, csn, rip, rin), 0, N)
    W = tcsc_amd.TcscMatrix.from_arrays(K, N, csp, csn, rip, rin)
    with pytest.raises(tcsc_amd.TcscError, match=r"status 1\)"):
        tcsc_amd.Plan.transposed(W)
    W.free()
