"""_lib.Replay on the CPU: the eager / recorded / replayed rule of the decoders, with a stub engine (lib, prof, scratch_epoch) and
bodies that make no recordable call -- an empty finished CommandList runs without a device."""
import pytest


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as ge
    return ge.build()


class _Eng:
    def __init__(self):
        self.lib, self.prof, self.scratch_epoch = object(), None, 0


class _Body:
    """counts its calls and notes what stood in for eng.lib during each"""

    def __init__(self, eng, during=None):
        self.eng, self.calls, self.libs, self.during = eng, 0, [], during

    def __call__(self):
        self.calls += 1
        self.libs.append(self.eng.lib)
        if self.during is not None:
            self.during()


def _sight(replay, eng, key, body, unit=0):
    replay.begin(eng, key)(unit, body)


def test_eager_then_recorded_then_replayed(built):
    L = built._lib
    eng, rp = _Eng(), L.Replay(4)
    real, body = eng.lib, _Body(eng)
    counts, recorded = [], []
    for _ in range(4):
        _sight(rp, eng, 'k', body)
        assert eng.lib is real
        counts.append(body.calls)
        recorded.append(len(rp.recorded()))
    assert counts == [1, 2, 2, 2]                            # sightings 3 and 4 run the list, not the body
    assert recorded == [0, 1, 1, 1]
    assert body.libs[0] is real and isinstance(body.libs[1], L.Recorder)
    assert rp.keys() == ['k'] and rp.recorded('k') == rp.recorded() and rp.recorded('other') == []
    assert isinstance(rp.recorded()[0], L.CommandList) and rp.recorded()[0].n == 0


def test_a_body_that_raises_while_recording_leaves_nothing_behind(built):
    L = built._lib
    eng, rp = _Eng(), L.Replay(4)
    real = eng.lib

    def boom():
        if isinstance(eng.lib, L.Recorder):
            raise KeyError('inside the recording')
    body = _Body(eng, during=boom)
    _sight(rp, eng, 'k', body)
    with pytest.raises(KeyError):
        _sight(rp, eng, 'k', body)
    assert eng.lib is real and rp.recorded() == [] and body.calls == 2


@pytest.mark.parametrize('how', ['prof', 'recorder'])
def test_bypass_runs_the_body_and_changes_nothing(built, how):
    L = built._lib
    eng, rp = _Eng(), L.Replay(4)
    if how == 'prof':
        eng.prof = object()
    else:
        eng.lib = L.Recorder(object(), L.CommandList())
    standing = eng.lib
    body = _Body(eng)
    for n in range(1, 5):
        _sight(rp, eng, 'k', body)
        assert body.calls == n and eng.lib is standing
    assert all(lib is standing for lib in body.libs)
    assert rp.keys() == [] and rp.recorded() == []
    # ... also for a key that has a list already: the body runs, the list stays
    eng.lib, eng.prof = object(), None
    _sight(rp, eng, 'k', body)
    _sight(rp, eng, 'k', body)
    assert len(rp.recorded('k')) == 1
    kept = rp.recorded('k')[0]
    eng.prof = object()
    _sight(rp, eng, 'k', body)
    assert body.calls == 7 and rp.recorded('k') == [kept]


def test_epoch_bump_between_sightings_starts_the_key_over(built):
    L = built._lib
    eng, rp = _Eng(), L.Replay(4)
    body = _Body(eng)
    for _ in range(3):
        _sight(rp, eng, 'k', body)
    assert body.calls == 2 and len(rp.recorded('k')) == 1
    old = rp.recorded('k')[0]
    eng.scratch_epoch += 1
    _sight(rp, eng, 'k', body)                               # eager again
    assert body.calls == 3 and rp.recorded('k') == [] and body.libs[-1] is eng.lib
    _sight(rp, eng, 'k', body)                               # recorded again
    assert body.calls == 4 and len(rp.recorded('k')) == 1 and rp.recorded('k')[0] is not old
    assert isinstance(body.libs[-1], L.Recorder)
    _sight(rp, eng, 'k', body)
    assert body.calls == 4 and rp.keys() == ['k']


def test_epoch_bump_inside_the_recording_keeps_no_list(built):
    L = built._lib
    eng, rp = _Eng(), L.Replay(4)

    def bump():
        if isinstance(eng.lib, L.Recorder):
            eng.scratch_epoch += 1
    body = _Body(eng, during=bump)
    _sight(rp, eng, 'k', body)
    _sight(rp, eng, 'k', body)
    assert body.calls == 2 and rp.recorded() == [] and eng.scratch_epoch == 1


def test_epoch_bump_between_units_makes_the_rest_of_the_search_eager(built):
    L = built._lib
    eng, rp = _Eng(), L.Replay(4)
    body = _Body(eng)
    for _ in range(2):                                       # units 0..2 seen once, then recorded
        run = rp.begin(eng, 'k')
        for u in range(3):
            run(u, body)
    assert body.calls == 6 and len(rp.recorded('k')) == 3
    run = rp.begin(eng, 'k')
    run(0, body)                                             # replayed
    assert body.calls == 6
    eng.scratch_epoch += 1
    real = eng.lib
    run(1, body)
    run(2, body)
    run(3, body)                                             # (a unit this key has never seen: eager as well, and not noted)
    assert body.calls == 9 and body.libs[-3:] == [real] * 3 and eng.lib is real
    assert len(rp.recorded('k')) == 3                        # nothing recorded, nothing dropped by that search ...
    run = rp.begin(eng, 'k')                                 # ... the next lookup starts the key over
    run(3, body)
    assert rp.recorded('k') == [] and body.libs[-1] is real


@pytest.mark.parametrize('capacity', [2, 4])
def test_a_key_beyond_the_capacity_evicts_the_oldest(built, capacity):
    L = built._lib
    eng, rp = _Eng(), L.Replay(capacity)
    body = _Body(eng)
    keys = ['k%d' % i for i in range(capacity)]
    for k in keys:
        _sight(rp, eng, k, body)
        _sight(rp, eng, k, body)
    assert rp.keys() == keys and len(rp.recorded()) == capacity
    _sight(rp, eng, keys[0], body)                           # a replay of the oldest key does not make it younger
    _sight(rp, eng, 'new', body)
    assert rp.keys() == keys[1:] + ['new'] and rp.recorded(keys[0]) == []
    assert len(rp.recorded()) == capacity - 1
    calls = body.calls
    _sight(rp, eng, keys[0], body)                           # the evicted key is at its first sighting again, and evicts the next oldest
    assert body.calls == calls + 1 and body.libs[-1] is eng.lib
    assert rp.keys() == keys[2:] + ['new', keys[0]]


def test_units_of_one_key_are_independent(built):
    L = built._lib
    eng, rp = _Eng(), L.Replay(2)
    body0, body4 = _Body(eng), _Body(eng)
    for _ in range(2):
        _sight(rp, eng, 'k', body0, unit=0)
    run = rp.begin(eng, 'k')
    run(0, body0)                                            # replayed ...
    run(4, body4)                                            # ... while unit 4 is at its first sighting
    assert body0.calls == 2 and body4.calls == 1 and body4.libs == [eng.lib]
    assert len(rp.recorded('k')) == 1
    run(4, body4)
    assert isinstance(body4.libs[-1], L.Recorder) and len(rp.recorded('k')) == 2
    run(4, body4)
    assert body4.calls == 2
