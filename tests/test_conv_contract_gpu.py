"""conv_gemm's contract as the extension exports it (csrc/include/psamd_launch.h ConvEpi and the
host predicates next to the launch ladders) against its Python side (ps_amd/ops/convgemm.py).

Host-side checks only: no kernel is launched (marked gpu because ps_amd._C loads there)."""
import pytest
import torch

from ps_amd.ops import native
from ps_amd.ops.convgemm import Epi, geo

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_epi_names_match_extension():
    assert dict(Epi.__members__) == native().EPI
    assert sorted(native().EPI.values()) == list(range(10))


def test_twosrc_glds_threshold_exported():
    assert native().kTwosrcGldsMinNk == 4


# (h, w, stride, c1 -> c2, expected) from the 3x3 patch weight-gradient kernel's shapes: pad 1,
# stride 1 on 56- / 28-wide maps of whole 112-pixel stages, stride 2 on a 56-wide map with
# h % 8 == 0, c1 <= 128, channels multiples of 64
_PATCH_TABLE = [
    (56, 56, 1, 64, 64, True),
    (28, 28, 1, 128, 128, True),
    (56, 56, 2, 128, 128, True),
    (14, 14, 1, 256, 256, False),
    (56, 56, 1, 192, 192, False),
    (57, 56, 1, 64, 64, False),
    (60, 56, 2, 128, 128, False),
    (56, 56, 3, 64, 64, False),
]


@pytest.mark.parametrize("images", [1, 2])
@pytest.mark.parametrize("h,w,s,c1,c2,want", _PATCH_TABLE)
def test_conv_wgrad_patch_ok_truth_table(h, w, s, c1, c2, want, images):
    assert native().conv_wgrad_patch_ok(geo(h, w, 3, s, 1), images, c2, c1) is want


def test_fold_ds_epilogue_rejected_on_tall_tile():
    """Epi.FOLD_ADD_MASKED_DS has no 256 x 64 kernel: the argument check raises before any launch
    (every tensor the epilogue needs is supplied at its size, so it is that check that fires)."""
    M, C, N = 256, 512, 64
    gg = [M, 1, M, 1, 1, 1, 0]
    assert native().conv_gemm_plan(M, N, C, gg, False, int(Epi.FOLD_ADD_MASKED_DS))[:2] == [256, 64]
    rows = lambda: torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)  # noqa: E731
    bits = lambda: torch.zeros(M * N // 8, dtype=torch.uint8, device=DEV)  # noqa: E731
    vec = lambda: torch.ones(N, dtype=torch.float32, device=DEV)  # noqa: E731
    a = torch.zeros(M, C, dtype=torch.bfloat16, device=DEV)
    b = torch.zeros(N, C, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match=r"256 x 64 tiles planned for this shape have no kernel .* epilogue 9"):
        native().conv_gemm(a, b, gg, epi=Epi.FOLD_ADD_MASKED_DS, aux=rows(), bits=bits(), aux2=rows(), bits2=bits(),
                           mean=vec(), invstd=vec(), aux3=rows(), mean2=vec(), invstd2=vec())
