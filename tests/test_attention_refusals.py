"""CPU-side refusals of the relative-attention forward and backward entry points: every check here runs on the host
before anything is launched, so each call returns without touching a device.  One fault per call; the return code and
the full text of isi_last_error() are pinned, for isi_rel_attention_f32 ("rel_attention: ...") and for
isi_rel_attention_bwd_f32 ("rel_attention_bwd: ...").

No case reaches "band too wide": the check is 127 / Cq + 31 / Ck + 1 > 160 (the backward also tests the form with Cq and Ck
swapped), the event-layout check in front of it has already refused Cq <= 0 and Ck <= 0, and with Cq, Ck >= 1 the integer
quotients are at most 127 and 31, so the sum is at most 159 whatever the sizes."""
import ctypes

import pytest

INVALID, UNSUPPORTED = -1, -4
FWD, BWD = "rel_attention", "rel_attention_bwd"
ALIGNMENT = "strides must be multiples of 4 floats and pointers 16-byte aligned"
STRIDES = [t + s for t in "qkvo" for s in ("_ss", "_sb", "_sh")]

_BACKING = (ctypes.c_char * 64)()
PLACEHOLDER = (ctypes.addressof(_BACKING) + 15) & ~15   # 16-byte aligned host memory, never dereferenced


def _args():
    """A call with no fault (Sq = Sk = 8, B = 1, H = 2, head_dim 16, one channel per event): every case below breaks ONE
    thing in it.  Unbroken it would be launched, so it is never passed on as it is."""
    from interactive_spectrogram_inpainting import _hip
    a = _hip.isi_attn_bwd_args()
    g = a.fwd
    g.q = g.k = g.v = g.out = g.rel_embeddings = g.lse = PLACEHOLDER
    g.Sq, g.Sk, g.B, g.H, g.head_dim = 8, 8, 1, 2, 16
    for s in STRIDES:
        setattr(g, s, 16 if s.endswith("_sh") else 32)
    g.Cq, g.Ck, g.Ek, g.rel_rows = 1, 1, 8, 15
    g.mask_mode, g.scale, g.precision = 0, 0.25, 0
    a.d_out = a.dq = a.dk = a.dv = a.d_rel = a.workspace = PLACEHOLDER
    a.workspace_floats = 1 << 40
    return a


def _call(who, a):
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()
    if who == FWD:
        rc = lib.isi_rel_attention_f32(ctypes.byref(a.fwd), None)
    else:
        rc = lib.isi_rel_attention_bwd_f32(ctypes.byref(a), None)
    return rc, lib.isi_last_error().decode()


def _refused(who, a, code, text):
    assert _call(who, a) == (code, f"{who}: {text}")


both = pytest.mark.parametrize("who", [FWD, BWD])


@both
@pytest.mark.parametrize("field", ["q", "k", "v", "out"])
def test_null_pointer(who, field):
    a = _args()
    setattr(a.fwd, field, None)
    _refused(who, a, INVALID, "null pointer")


@both
def test_null_argument_struct(who):
    from interactive_spectrogram_inpainting import _hip
    lib = _hip.lib()
    rc = lib.isi_rel_attention_f32(None, None) if who == FWD else lib.isi_rel_attention_bwd_f32(None, None)
    assert (rc, lib.isi_last_error().decode()) == (INVALID, f"{who}: null pointer")


@both
@pytest.mark.parametrize("field,value", [("Sq", 0), ("Sk", 0), ("B", 0), ("H", 0), ("Sq", -3)])
def test_non_positive_shape(who, field, value):
    a = _args()
    setattr(a.fwd, field, value)
    _refused(who, a, INVALID, "bad shape")


@both
@pytest.mark.parametrize("field,value", [("Cq", 0), ("Ck", 0), ("Ek", 0), ("Ck", -1)])
def test_bad_event_layout(who, field, value):
    a = _args()
    setattr(a.fwd, field, value)
    _refused(who, a, INVALID, "bad event layout")


@both
@pytest.mark.parametrize("mode", [-1, 3])
def test_mask_mode_out_of_range(who, mode):
    a = _args()
    a.fwd.mask_mode = mode
    _refused(who, a, INVALID, "bad mask mode")


@both
@pytest.mark.parametrize("tensor", list("qkvo"))
def test_span_over_4_gib_through_strides(who, tensor):
    """(S - 1) ss + (B - 1) sb + (H - 1) sh + head_dim floats, with a sequence stride of 2^30: 4 GiB + 128 bytes, no
    allocation behind it."""
    a = _args()
    setattr(a.fwd, tensor + "_ss", 1 << 30)
    _refused(who, a, UNSUPPORTED, "tensor spans 4 GiB or more")


@both
@pytest.mark.parametrize("stride", STRIDES)
def test_stride_not_a_multiple_of_4(who, stride):
    a = _args()
    setattr(a.fwd, stride, getattr(a.fwd, stride) + 2)
    _refused(who, a, INVALID, ALIGNMENT)


@both
@pytest.mark.parametrize("field", ["q", "k", "v", "out", "rel_embeddings"])
def test_misaligned_pointer(who, field):
    a = _args()
    setattr(a.fwd, field, PLACEHOLDER + 4)
    _refused(who, a, INVALID, ALIGNMENT)


@pytest.mark.parametrize("precision", [-1, 4])
def test_forward_precision_out_of_range(precision):
    a = _args()
    a.fwd.precision = precision
    _refused(FWD, a, INVALID, "precision must be 0 .. 3")


def test_backward_rel_rows_or_d_rel_missing():
    a = _args()
    a.d_rel = None
    _refused(BWD, a, INVALID, "rel_rows / d_rel missing")
    a = _args()
    a.fwd.rel_rows = 0
    _refused(BWD, a, INVALID, "rel_rows / d_rel missing")


# what the backward refuses on top of the common part, with the common part's texts
@pytest.mark.parametrize("field", ["d_out", "dq", "dk", "dv", "workspace"])
def test_backward_own_pointers(field):
    a = _args()
    setattr(a, field, None)
    _refused(BWD, a, INVALID, "null pointer")
    a = _args()
    setattr(a, field, PLACEHOLDER + 4)
    _refused(BWD, a, INVALID, ALIGNMENT)


def test_backward_needs_lse():
    a = _args()
    a.fwd.lse = None
    _refused(BWD, a, INVALID, "null pointer")
