"""ltp_row_line (include/ltp_hip.h): how much of a dense row the samplers write — the stored samples rounded up to whole 64-byte
lines — against ltp_row_stride, the row's padded length. No device needed."""
import pytest


@pytest.fixture(scope="module")
def lib():
    from longtermplanner_amd import _abi
    _abi.build()
    return _abi.lib()


@pytest.mark.parametrize("element_bytes", [8, 4])
def test_row_line_rounds_up_to_lines_inside_the_row(lib, element_bytes):
    per_line = 64 // element_bytes                      # 8 doubles, 16 floats
    for n in range(0, 601):
        line, stride = lib.ltp_row_line(n, element_bytes), lib.ltp_row_stride(n)
        assert line == (n + per_line - 1) // per_line * per_line, n
        assert n <= line < n + per_line and line % per_line == 0, n
        assert line <= stride, n                        # the zeros never leave the row
        assert stride % per_line == 0, n                # rows start on a line
        if n % per_line == 0:
            assert line == n, n                         # a whole-line row gets nothing added


def test_row_line_of_nothing(lib):
    assert lib.ltp_row_line(0, 8) == 0 and lib.ltp_row_line(-5, 4) == 0
    assert lib.ltp_row_line(100, 2) == 0 and lib.ltp_row_line(100, 16) == 0      # not an element size of a row
