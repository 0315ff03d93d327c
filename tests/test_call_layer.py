"""CPU: the helpers every Python call site reaches liblde.so through (_lib.ptr / ptr_array / call / NativeModule / hand_over_weights),
driven with a fake library — plain Python callables that record their arguments — so nothing here touches HIP."""
import ctypes as C

import pytest
import torch

from latentdiffeq_amd import _lib as L


class FakeLib:
    """Records (name, args) per call; `rc[name]` is the status a call returns (0 by default)."""

    def __init__(self, **rc):
        self.calls, self.rc = [], rc
        for kind in ("chain_", "rnn_", ""):
            setattr(self, f"lde_{kind}last_error", lambda h, kind=kind: f"text of lde_{kind}last_error".encode())

    def __getattr__(self, name):
        if not name.startswith("lde_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return self.rc.get(name, 0)
        return fn

    def names(self):
        return [n for n, _ in self.calls]


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(L, "_lib", lib)          # load() returns it; check() asks it for the error text
    return lib


def test_ptr_and_ptr_array():
    t = torch.arange(6, dtype=torch.float32)
    assert L.ptr(None).value is None
    assert L.ptr(t).value == t.data_ptr() and L.ptr(t, 4).value == t.data_ptr() + 4
    u = torch.zeros(3)
    arr = L.ptr_array([u, None, t, 12345, L.ptr(t, 8).value])
    assert isinstance(arr, C.c_void_p * 5)
    assert list(arr) == [u.data_ptr(), None, t.data_ptr(), 12345, t.data_ptr() + 8]
    assert len(L.ptr_array([])) == 0


@pytest.mark.parametrize("name, source", [("lde_chain_forward", "lde_chain_last_error"), ("lde_rnn_forward_train", "lde_rnn_last_error"),
                                          ("lde_forward", "lde_last_error")])
def test_call_names_the_called_function_and_asks_the_right_error_source(fake, name, source):
    h = C.c_void_p(77)
    L.call(name, h, 1, 2)                                     # status 0: passes, the handle goes first
    assert fake.calls == [(name, (h, 1, 2))]
    fake.rc[name] = -2
    with pytest.raises(L.LdeError) as e:
        L.call(name, h, 3)
    assert str(e.value) == f"{name} failed: LDE_ERR_UNSUPPORTED: text of {source}"


def test_call_without_a_handle_and_with_an_error_handle(fake):
    L.call("lde_mse_forward", None, 5, 6)
    assert fake.calls == [("lde_mse_forward", (5, 6))]
    fake.rc.update(lde_mse_forward=-1, lde_rnn_group_forward_train=-1)
    with pytest.raises(L.LdeError) as e:
        L.call("lde_mse_forward", None, 5, 6)
    assert str(e.value) == "lde_mse_forward failed: LDE_ERR_INVALID_ARG"          # no handle: the status alone
    with pytest.raises(L.LdeError) as e:
        L.call("lde_rnn_group_forward_train", None, 3, err=C.c_void_p(9))       # a group call: the handle is not an argument
    assert fake.calls[-1] == ("lde_rnn_group_forward_train", (3,))
    assert str(e.value) == "lde_rnn_group_forward_train failed: LDE_ERR_INVALID_ARG: text of lde_rnn_last_error"


class _Owner(L.NativeModule):
    _create, _destroy = "lde_chain_create", "lde_chain_destroy"
    num_weights = 4

    def __init__(self):
        self.hooks = 0

    def _desc(self):
        return L.ChainDesc()

    def _created(self, h):
        self.hooks += 1


def _creating(lib, value, rc=0):
    def create(desc, out):
        lib.calls.append(("lde_chain_create", ()))
        out._obj.value = value
        return rc
    lib.lde_chain_create = create


def test_native_module_creates_once_and_destroys_once(fake):
    _creating(fake, 1234)
    m = _Owner()
    assert m._handle is None and m._lib is None and m._wkey is None and not m._is_recurrent
    h = m._native()
    assert h.value == 1234 and m._native() is h and m._handle is h and m._lib is fake
    assert fake.names() == ["lde_chain_create"] and m.hooks == 1
    m.__del__()
    m.__del__()
    assert fake.names() == ["lde_chain_create", "lde_chain_destroy"] and fake.calls[-1][1][0] is h


def test_native_module_destroys_a_half_made_handle_and_swallows_errors_in_del(fake):
    _creating(fake, 555, rc=-6)
    m = _Owner()
    with pytest.raises(L.LdeError, match="lde_chain_create failed: LDE_ERR_ALLOC: text of lde_chain_last_error"):
        m._native()
    assert fake.names() == ["lde_chain_create", "lde_chain_destroy"] and fake.calls[-1][1][0].value == 555
    assert m._handle is None and m.hooks == 0
    m.__del__()                                                  # nothing to destroy
    assert fake.names().count("lde_chain_destroy") == 1
    _creating(fake, None, rc=-3)                                 # a NULL handle: nothing to destroy, no handle to ask
    with pytest.raises(L.LdeError, match=r"lde_chain_create failed: LDE_ERR_NO_DEVICE$"):
        _Owner()._native()
    assert fake.names().count("lde_chain_destroy") == 1
    _creating(fake, 99)
    m = _Owner()
    m._native()

    def boom(h):
        raise RuntimeError("destroy failed")
    fake.lde_chain_destroy = boom
    m.__del__()                                                  # swallowed


def test_hand_over_weights_uploads_only_what_the_handle_does_not_hold(fake):
    _creating(fake, 42)
    m = _Owner()
    W = torch.arange(4, dtype=torch.float32)
    stream = C.c_void_p(7)
    h = L.hand_over_weights(m, W, stream)
    assert h is m._handle and m._wkey is None
    name, (h_, p, n, s) = fake.calls[-1]
    assert (name, h_, p.value, n, s) == ("lde_chain_set_weights_device", h, W.data_ptr(), 4, stream)
    m._wkey = L.weights_key(W)                                   # what refresh_weights() leaves behind
    before = len(fake.calls)
    assert L.hand_over_weights(m, W, stream) is h
    assert len(fake.calls) == before and m._wkey == L.weights_key(W)
    W.add_(1.0)                                                  # an in-place update: the key no longer matches
    L.hand_over_weights(m, W, stream)
    assert len(fake.calls) == before + 1 and m._wkey is None
    m._is_recurrent = True
    L.hand_over_weights(m, W, stream)
    assert fake.names()[-1] == "lde_rnn_set_weights_device"


def test_hand_over_weights_converts_before_taking_the_pointer(fake):
    _creating(fake, 42)
    m = _Owner()
    seen = []

    def upload(h, p, n, s):
        seen.append((C.c_float * n).from_address(p.value)[:])    # what the library would read, while the call is in flight
        return 0
    fake.lde_chain_set_weights_device = upload
    base = torch.arange(8, dtype=torch.float64)
    L.hand_over_weights(m, base[::2], None)                      # neither contiguous nor f32
    L.hand_over_weights(m, torch.tensor([1, 2, 3, 4], dtype=torch.int32), None)
    assert seen == [[0.0, 2.0, 4.0, 6.0], [1.0, 2.0, 3.0, 4.0]]


def test_small_shared_pieces():
    a, b, c = torch.ones(2), torch.full((2,), 2.0), torch.full((2,), 4.0)
    assert L.sum_gradients(None) is None and L.sum_gradients([a]) is a
    assert torch.equal(L.sum_gradients([a, b, c]), torch.full((2,), 7.0))
    ws, p0, p1 = L.loss_scratch("cpu", 3)
    assert ws.shape == (4,) and ws.dtype == torch.float32 and (p0.value, p1.value) == (ws.data_ptr(), ws.data_ptr() + 4)
    assert L.loss_scratch("cpu")[0].numel() == L.LOSS_SCRATCH_FLOATS + 1
    dW = L.new_weight_gradient(_Owner(), "cpu")                   # (no weight-gradient stream set: nothing to record)
    assert dW.shape == (4,) and dW.dtype == torch.float32 and L.dw_stream is None
    L.need_gpu(True, "x")
    with pytest.raises(L.LdeError, match="no CPU fallback"):
        L.need_gpu(False, "Chain")
