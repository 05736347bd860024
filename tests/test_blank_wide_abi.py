"""Blank-CTC loss on lattices wider than one wave (256 <= S <= 1023 labels): the workspace size and the shape limit of
the C ABI (runs without a GPU).  tests/test_blank_wide_gpu.py checks the kernels."""
import pytest

BLANK = 2


@pytest.fixture(scope="module")
def lib():
    from ctc_amd import _lib, build
    build.build()
    return _lib.load()


@pytest.mark.parametrize("S", [256, 511, 512, 1023])
def test_workspace_covers_the_wide_lattice(lib, S):
    T, B, C = 1250, 2, 20
    assert lib.ctc_amd_workspace_bytes(BLANK, T, B, C, S) >= 256 + 3 * B * T * (2 * S + 1) * 4


def test_workspace_grows_with_the_labels(lib):
    sizes = [lib.ctc_amd_workspace_bytes(BLANK, 700, 3, 40, S) for S in range(1, 1024)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))


# ctc_amd_workspace_bytes of the library before the wide path, read from a build of it: the read-outs size
# themselves against these, and nothing changes at S <= 255
@pytest.mark.parametrize("shape, size", [((2000, 64, 1000, 100), 393446144), ((300, 6, 400, 60), 2791680),
                                         ((2000, 4, 600, 255), 49195008)])
def test_narrow_workspace_unchanged(lib, shape, size):
    assert lib.ctc_amd_workspace_bytes(BLANK, *shape) == size


@pytest.mark.parametrize("S", [1024, 5000])
def test_too_many_labels(lib, S):
    # rejected before anything is dereferenced or launched: the pointers are non-null but bogus
    p = 16
    rc = lib.ctc_amd_blank_loss_grad(p, 0, 0, p, 0, p, p, 4, 2, 1000, S, 0, 1.0, 1.0, p, p, p, p, None)
    assert rc == -2
