"""The argument handling the five wrappers of the generative side share in evcouplings_amd/plm.py (sample, log_partition,
parallel_tempering, anneal, bm_fit), without a GPU: the exact text of every ValueError for a wrong model, start, fixed
or allowed argument, and the callback trampoline, with the library replaced by a stub that calls the callback once."""
import numpy as np
import pytest

from evcouplings_amd import _lib, plm

L, Q, CH = 4, 3, 8
N_J = L * (L - 1) // 2


def _model(L=L, q=Q):
    rng = np.random.default_rng(1)
    return rng.normal(size=(L, q)).astype(np.float32), rng.normal(size=(L * (L - 1) // 2, q, q)).astype(np.float32)


def _sample(h, J, **kw):
    return plm.sample(h, J, Q, CH, **kw)


def _log_partition(h, J, **kw):
    return plm.log_partition(h, J, Q, n_chains=CH, n_temps=4, **kw)


def _parallel_tempering(h, J, **kw):
    return plm.parallel_tempering(h, J, Q, CH, np.array([0.0, 0.5, 1.0], np.float32), **kw)


def _anneal(h, J, **kw):
    return plm.anneal(h, J, Q, CH, n_steps=3, **kw)


def _bm_fit(h, J, **kw):
    fi = np.full((L, Q), 1.0 / Q, np.float32)
    fij = np.full((N_J, Q, Q), 1.0 / (Q * Q), np.float32)
    return plm.bm_fit(fi, fij, Q, h, J, CH, 2, **kw)


WRAPPERS = dict(sample=_sample, log_partition=_log_partition, parallel_tempering=_parallel_tempering, anneal=_anneal,
                bm_fit=_bm_fit)


def _raises(text, call, *args, **kw):
    with pytest.raises(ValueError) as err:
        call(*args, **kw)
    assert str(err.value) == text


@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_a_wrong_model_is_refused_in_the_same_words_by_every_wrapper(name):
    call = WRAPPERS[name]
    h, J = _model()
    hi_text = "hi must be an (L, q) matrix with q = 3"
    _raises(hi_text, call, h.reshape(-1), J)                     # not a matrix
    _raises(hi_text, call, h[:, :2], J)                          # q - 1 columns
    _raises(hi_text, call, np.zeros((0, Q), np.float32), J)      # no site
    _raises("jij has 45 entries, expected the 6 i<j blocks of 3 x 3", call, h, J[:-1])
    _raises("jij has 63 entries, expected the 6 i<j blocks of 3 x 3", call, h, np.zeros(63, np.float32))


@pytest.mark.parametrize("name", ["sample", "anneal", "bm_fit"])
def test_a_wrong_start_shape(name):
    h, J = _model()
    text = "start must be an (n_chains, L) = (8, 4) matrix of states"
    _raises(text, WRAPPERS[name], h, J, start=np.zeros((CH - 1, L), np.int8))
    _raises(text, WRAPPERS[name], h, J, start=np.zeros((CH, L + 1), np.int8))
    _raises(text, WRAPPERS[name], h, J, start=np.zeros(CH * L, np.int8))


def test_a_wrong_start_of_parallel_tempering():
    h, J = _model()
    _raises("the start states must be an (n_ladders * R, L) = (24, 4) matrix", _parallel_tempering, h, J,
            start=(np.zeros((23, L), np.int8),))
    _raises("start must be (states, rungs, e_j), (states, rungs) or (states,)", _parallel_tempering, h, J, start=())
    _raises("the start rungs must hold n_ladders * R = 24 values", _parallel_tempering, h, J,
            start=(np.zeros((24, L), np.int8), np.zeros(23, np.int32)))
    _raises("start energies need the start rungs", _parallel_tempering, h, J,
            start=(np.zeros((24, L), np.int8), None, np.zeros(24)))
    _raises("the start energies must hold n_ladders * R = 24 values", _parallel_tempering, h, J,
            start=(np.zeros((24, L), np.int8), np.zeros(24, np.int32), np.zeros(23)))


@pytest.mark.parametrize("name", ["sample", "anneal"])
def test_wrong_fixed_and_allowed_lengths(name):
    h, J = _model()
    for bad in (np.zeros(L - 1), np.zeros(L + 1), np.zeros((1, L))):
        _raises("fixed must hold L = 4 flags", WRAPPERS[name], h, J, fixed=bad)
    for bad in (np.ones(Q - 1), np.ones(Q + 1), np.ones((1, Q))):
        _raises("allowed must hold q = 3 flags", WRAPPERS[name], h, J, allowed=bad)


def test_the_order_of_the_checks():
    """The model comes first, then the wrapper's own scalars, then start, fixed, allowed in that order."""
    h, J = _model()
    bad = dict(start=np.zeros((1, 1), np.int8), fixed=np.zeros(1), allowed=np.zeros(1))
    for name in ("sample", "anneal"):
        _raises("jij has 45 entries, expected the 6 i<j blocks of 3 x 3", WRAPPERS[name], h, J[:-1], **bad)
        _raises("start must be an (n_chains, L) = (8, 4) matrix of states", WRAPPERS[name], h, J, **bad)
        _raises("fixed must hold L = 4 flags", WRAPPERS[name], h, J, fixed=bad["fixed"], allowed=bad["allowed"])
    _raises("need n_chains >= 1, n_snapshots >= 1, burn_in >= 0 and thin >= 1", plm.sample, h, J, Q, 0, **bad)
    _raises("need n_chains >= 1", plm.anneal, h, J, Q, 0, **bad)


class _StubLibrary:
    """Every entry point with a callback calls it once, records what it answered and reports success."""

    def __init__(self):
        self.answers = []

    def _progress(self, *args):
        cb = args[-3]
        if cb:                                                   # a NULL function pointer is false
            self.answers.append(cb(1, 2, None))
        return 0

    plm_ais = plm_pt = plm_anneal = _progress

    def plm_bm_fit(self, *args):
        cb = args[-3]
        if cb:
            self.answers.append(cb(0, 0.125, 0.25, 0.5, 0.75, None))
        return 0


@pytest.fixture
def stub(monkeypatch):
    lib = _StubLibrary()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    return lib


class _Stop(Exception):
    pass


@pytest.mark.parametrize("name", ["log_partition", "parallel_tempering", "anneal", "bm_fit"])
def test_an_exception_of_the_callback_is_raised_again_by_the_wrapper(stub, name):
    h, J = _model()
    seen = []

    def callback(*args):
        seen.append(args)
        raise _Stop(name)

    with pytest.raises(_Stop) as err:
        WRAPPERS[name](h, J, callback=callback)
    assert str(err.value) == name
    assert stub.answers == [1]                                   # the library is told to stop
    want = (0, 0.125, 0.25, 0.5, 0.75) if name == "bm_fit" else (1, 2)
    assert seen == [want] and all(type(a) is type(b) for a, b in zip(seen[0], want))


def test_the_callback_answer_and_the_missing_callback(stub):
    """A true value stops, a false one goes on, and no callback is a NULL pointer the library never calls."""
    h, J = _model()
    for answer, want in ((True, 1), (0, 0), (None, 0), ("stop", 1)):
        del stub.answers[:]
        _anneal(h, J, callback=lambda done, total: answer)
        _bm_fit(h, J, callback=lambda epoch, d_i, d_ij, rms, lr: answer)
        _log_partition(h, J, betas=[0.0, 0.5], callback=lambda done, total: answer)
        assert stub.answers == [want] * 3
    del stub.answers[:]
    _anneal(h, J)
    _bm_fit(h, J)
    _log_partition(h, J, betas=[0.0, 0.5])
    assert stub.answers == []
