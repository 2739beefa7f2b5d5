"""TEST INFRASTRUCTURE: tests/oracle_batch.py's host-only stand-in for LDSBatch, with the per-replicate bookkeeping of the
real handle on top -- set_active / active / status (pyvb_amd/lds.py) -- so that what pyvb_amd/_recognise.py: LDSGroup does
with them can be exercised without a GPU:

  * rows that are switched off are restored after every oracle call (the oracle itself computes every row), so they read
    back as they were, as on the device; `frozen[r]` keeps what row r held when it was switched off;
  * a test can declare "row r fails at the k-th sweep" (MaskedOracleBatch.fail_next = (r, k) before the handle is made):
    that sweep leaves garbage in the row and raises its status flag; the next call that would synchronise the real handle
    (get_state, get_posterior_classes, get_column_qld, elbo) raises LinAlgError once and clears the flag, as pyvb_lds_sync
    does, unless the row has been switched off; status() reports pending and just-reported flags.
Nothing under pyvb_amd/ imports this file.
"""
import numpy as np

from oracle_batch import OracleBatch

FAIL_STATES = 1
GARBAGE = 12345.0


class MaskedOracleBatch(OracleBatch):
    fail_next = None                # (row, number of the sweep that fails, from 1): taken by the next handle that is made

    def __init__(self, N, T, D, K, noise="diagonal_gamma", device=0):
        OracleBatch.__init__(self, N, T, D, K, noise, device)
        self._active = np.ones(N, dtype=bool)
        self._pending = np.zeros(N, dtype=np.int32)
        self._reported = np.zeros(N, dtype=np.int32)
        self._fail, type(self).fail_next = type(self).fail_next, None
        self._sweeps = 0
        self.frozen = {}

    # -- the mask --------------------------------------------------------------------------------
    def _rows(self):
        return {k: v for k, v in self.st.items() if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == self.N}

    def set_active(self, mask):
        mask = np.asarray(mask, dtype=bool)
        assert mask.shape == (self.N,)
        assert not (mask & ~self._active).any(), "PYVB_E_ARG: the mask can only shrink"
        for r in np.nonzero(self._active & ~mask)[0]:
            self.frozen[int(r)] = {k: v[r].copy() for k, v in self._rows().items()}
        self._active = mask.copy()
        self.log.append(("set_active", tuple(bool(m) for m in mask)))

    def active(self):
        return self._active.copy()

    def _masked(self, fn, *args):
        off = ~self._active
        keep = {k: v[off].copy() for k, v in self._rows().items()} if off.any() else {}
        out = fn(self, *args)
        for k, v in keep.items():
            self.st[k][off] = v
        return out

    def sweep(self, direction="forward"):
        self._masked(OracleBatch.sweep, direction)
        self._sweeps += 1
        if self._fail is not None and self._sweeps == self._fail[1] and self._active[self._fail[0]]:
            r = self._fail[0]
            self._pending[r] |= FAIL_STATES
            self.st["X"][r] = GARBAGE

    def update_columns(self, which, lo, hi):
        self._masked(OracleBatch.update_columns, which, lo, hi)

    def update_Q(self):
        self._masked(OracleBatch.update_Q)

    def update_R(self):
        self._masked(OracleBatch.update_R)

    # -- status ----------------------------------------------------------------------------------
    def _sync(self):
        if (self._pending != 0)[self._active].any():
            self._reported, self._pending = self._pending.copy(), np.zeros(self.N, dtype=np.int32)
            raise np.linalg.LinAlgError("a posterior precision was not positive definite")
        self._reported[:] = 0

    def status(self):
        return self._pending | self._reported

    def get_state(self, what=None):
        self._sync()
        return OracleBatch.get_state(self, what)

    def get_posterior_classes(self):
        self._sync()
        return OracleBatch.get_posterior_classes(self)

    def get_column_qld(self):
        self._sync()
        return OracleBatch.get_column_qld(self)

    def elbo(self):
        out = OracleBatch.elbo(self)
        self._sync()
        return out
