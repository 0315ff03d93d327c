"""What tests/test_gpu_sl.py and tests/test_gpu_sl_sde.py share: a handle of LDE_RHS_STUART_LANDAU, a test-owned dual record whose J can be
read back (n [B] | J [T][2N][B][G] | t, dt — include/lde.h: "the Stuart–Landau network"), and the parity gates. Test infrastructure only."""
import ctypes as C

import numpy as np

from tests import sl_ref as R


def native(N, **kw):
    from latentdiffeq_amd import _lib as L
    from tests.gpu_util import Native, make_desc
    return Native(make_desc(rhs_kind=L.RHS_STUART_LANDAU, state_dim=2 * N, param_dim=2 * N + 1, sensealg=L.SENSE_FORWARD_DUAL, **kw))


def fixed(N, solver, dt, **kw):
    return native(N, solver=solver, adaptive=0, dt=dt, **kw)


def set_noise(nat, seed=0, offset=0, first=0, epoch=None):
    from latentdiffeq_amd import _lib as L
    L.check(nat.lib.lde_set_noise(nat.h, seed, offset, first, C.c_void_p(epoch.data_ptr()) if epoch is not None else None), nat.h, "lde_set_noise")


def a256(x):
    return (x + 255) // 256 * 256


class Record:
    """A dual record owned by the test (lde_set_step_record), so that J can be read back."""

    def __init__(self, nat, N, B, T):
        import torch
        from latentdiffeq_amd import _lib as L
        self.nat, self.N, self.B, self.T = nat, N, B, T
        self.D, self.G = 2 * N, R.GROUP[N]
        self.nbytes = int(nat.lib.lde_step_record_bytes(nat.h, B, T))
        assert self.nbytes >= a256(4 * B) + a256(4 * T * self.D * B * self.G)
        self.buf = torch.zeros((self.nbytes,), device="cuda", dtype=torch.uint8)
        L.check(nat.lib.lde_set_step_record(nat.h, C.c_void_p(self.buf.data_ptr()), self.nbytes), nat.h, "lde_set_step_record")

    def n(self):
        import torch
        return self.buf[:4 * self.B].view(torch.int32).cpu().numpy()

    def JG(self):
        """[T, B, D, G]: the record's G columns, the pad lanes' included."""
        import torch
        off = a256(4 * self.B)
        raw = self.buf[off:off + 4 * self.T * self.D * self.B * self.G].view(torch.float32).cpu().numpy()
        return raw.reshape(self.T, self.D, self.B, self.G).transpose(0, 2, 1, 3).copy()


def rel(a, b):
    """max |a − b| relative to the largest entry of the reference array b (0 where both are all zero)."""
    m = np.abs(b).max()
    d = np.abs(np.asarray(a, np.float64) - b).max()
    return d / m if m > 0 else d


def gates(tag, z, J, g0, gth, zr, Jr, r0, rth, bounds=R.BOUNDS):
    ez, eJ, e0, eth = rel(z, zr), rel(J, Jr), rel(g0, r0), rel(gth, rth)
    print(f"{tag}: z {ez:.2e}, J {eJ:.2e}, dz0 {e0:.2e}, dtheta {eth:.2e} of the reference's largest entry (bounds {bounds})")
    assert ez <= bounds[0], ez
    assert eJ <= bounds[1], eJ
    assert e0 <= bounds[2] and eth <= bounds[3], (e0, eth)


def run(nat, N, z0, th, ts, dz):
    """forward into a test-owned record, J read back (the pad columns must be exact zeros), pullback."""
    D, P, NP = R.dims(N)
    B, T = z0.shape[0], len(ts)
    rec = Record(nat, N, B, T)
    z, ret, st = nat.forward(z0, th, ts)
    JG = rec.JG()
    assert (JG[..., NP:] == 0).all(), "the pad lanes' columns of the record are zero"
    g0, gth, _, sta = nat.adjoint(z, th, ts, dz)
    assert z.shape == (T, B, D) and g0.shape == (B, D) and gth.shape == (B, P)
    return dict(rec=rec, z=z, ret=ret, st=st, J=JG[..., :NP].copy(), g0=g0, gth=gth, sta=sta, n=rec.n())


def steps_of(tr):
    """The kernel's accepted steps (Native.step_record) as the reference's replay argument."""
    return [tr["t"][b, :tr["n"][b]] for b in range(len(tr["n"]))], [tr["dt"][b, :tr["n"][b]] for b in range(len(tr["n"]))]
