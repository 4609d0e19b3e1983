"""_lib.Replay on the CPU: the eager / recorded / replayed rule of the decoders, with a stub engine (lib, prof, scratch_epoch) and
bodies that make no recordable call -- an empty finished CommandList runs without a device.  Further down, what the trainer's
schedules add to it (eviction of the least recently used key, inputs that move between replays, on_break, clear()), with a stub library
handle that lets the Recorder log one call's real pointer arguments."""
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


# ---------------------------------------------------------------------------------------------------------------------
# what the trainer's schedules add: least-recently-used eviction, inputs that move between replays, on_break, clear()
# ---------------------------------------------------------------------------------------------------------------------
class _Handle:
    """stands in for the ctypes handle: one recordable name, whose call does nothing and succeeds -- the Recorder then logs real
    pointer arguments without a device"""

    def mtl_cmdlist_opcode(self, name):
        return 7 if name == b'mtl_axpy' else -1

    def mtl_axpy(self, *args):
        return 0


class _Axpy:
    """a body of one recordable call, mtl_axpy(stream, y, x, a, n), on the two addresses `at` holds at that moment"""

    def __init__(self, eng):
        self.eng, self.at, self.calls, self.libs = eng, None, 0, []

    def __call__(self):
        self.calls += 1
        self.libs.append(self.eng.lib)
        assert self.eng.lib.mtl_axpy(0x1000, self.at[0], self.at[1], 1.0, 4) == 0


A, B, C, D = 0x7f0000010000, 0x7f0000020000, 0x7f0000030000, 0x7f0000040000


@pytest.fixture
def ran(built, monkeypatch):
    """CommandList.run replaced by a note of (the pointer arguments y, x the list holds at that moment, the on_break it got)"""
    log = []
    monkeypatch.setattr(built._lib.CommandList, 'run', lambda self, on_break=None: log.append(
        ([self.buf[i].a[j].p for i in range(self.n) for j in (1, 2)], on_break)))
    return log


def _moving(L, **kw):
    eng = _Eng()
    eng.lib = _Handle()
    return eng, L.Replay(4, **kw), _Axpy(eng)


def _sight_at(rp, eng, body, at, inputs='at', on_break=None, key='k'):
    body.at = at
    rp.begin(eng, key)(0, body, inputs=at if inputs == 'at' else inputs, on_break=on_break)


@pytest.mark.parametrize('capacity', [2, 4])
def test_with_lru_a_replayed_oldest_key_survives_the_next_insertion(built, capacity):
    L = built._lib
    eng, rp = _Eng(), L.Replay(capacity, lru=True)
    body = _Body(eng)
    keys = ['k%d' % i for i in range(capacity)]
    for k in keys:
        _sight(rp, eng, k, body)
        _sight(rp, eng, k, body)
    assert rp.keys() == keys
    calls = body.calls
    _sight(rp, eng, keys[0], body)                           # a replay of the oldest key makes it the youngest
    assert body.calls == calls and rp.keys() == keys[1:] + [keys[0]]
    _sight(rp, eng, 'new', body)
    assert rp.keys() == keys[2:] + [keys[0], 'new'] and rp.recorded(keys[1]) == [] and len(rp.recorded(keys[0])) == 1
    _sight(rp, eng, keys[0], body)                           # ... and is still replayed
    assert body.calls == calls + 1


def test_inputs_that_change_between_replays_are_repointed(built, ran):
    eng, rp, body = _moving(built._lib)
    _sight_at(rp, eng, body, (A, B))
    _sight_at(rp, eng, body, (A, B))
    assert body.calls == 2 and isinstance(body.libs[1], built._lib.Recorder) and ran == []
    (cl,) = rp.recorded('k')
    assert cl.n == 1 and cl.buf[0].op == 7 and [cl.buf[0].a[j].p for j in range(3)] == [0x1000, A, B]
    _sight_at(rp, eng, body, (A, B))                         # the same addresses: as recorded
    _sight_at(rp, eng, body, (C, D))                         # both move
    _sight_at(rp, eng, body, (C, A))                         # one moves, onto an address the other once had
    _sight_at(rp, eng, body, (C, A))
    assert body.calls == 2 and [r[0] for r in ran] == [[A, B], [C, D], [C, A], [C, A]]
    assert cl.buf[0].a[0].p == 0x1000                        # (an argument that is no input stays)


def test_two_inputs_that_swap_addresses_end_up_swapped(built, ran):
    eng, rp, body = _moving(built._lib)
    for _ in range(3):
        _sight_at(rp, eng, body, (A, B))
    _sight_at(rp, eng, body, (B, A))
    _sight_at(rp, eng, body, (A, B))
    assert body.calls == 2 and [r[0] for r in ran] == [[A, B], [B, A], [A, B]]


def test_three_inputs_rotate_through_each_others_addresses(built, ran):
    L = built._lib
    eng = _Eng()
    eng.lib = _Handle()
    rp, at = L.Replay(4), [A, B, C]

    def body():                                              # two calls: (y, x) = (in0, in1), (in2, in0)
        assert eng.lib.mtl_axpy(0x1000, at[0], at[1], 1.0, 4) == 0 and eng.lib.mtl_axpy(0x1000, at[2], at[0], 1.0, 4) == 0
    for now in ([A, B, C], [A, B, C], [B, C, A], [C, A, B], [A, B, D]):
        at[:] = now
        rp.begin(eng, 'k')(0, body, inputs=tuple(at))
    assert [r[0] for r in ran] == [[B, C, A, B], [C, A, B, C], [A, B, D, A]]


def test_an_input_address_that_is_no_argument_of_the_list_raises(built, ran):
    eng, rp, body = _moving(built._lib)
    for _ in range(2):
        _sight_at(rp, eng, body, (A, B), inputs=(A, C))      # C is declared as an input, but the body never passes it
    with pytest.raises(KeyError):
        _sight_at(rp, eng, body, (A, B), inputs=(A, D))
    assert ran == []


def test_inputs_that_coincide_at_the_recording_sighting_run_eagerly_and_keep_no_list(built, ran):
    L = built._lib
    eng, rp, body = _moving(L)
    real = eng.lib
    _sight_at(rp, eng, body, (A, B))
    _sight_at(rp, eng, body, (A, A))                         # the second sighting would record: the inputs cannot be told apart
    assert body.calls == 2 and body.libs == [real, real] and rp.recorded() == [] and rp.keys() == ['k']
    _sight_at(rp, eng, body, (C, D))                         # the next sighting with distinct inputs records
    assert body.calls == 3 and isinstance(body.libs[2], L.Recorder) and len(rp.recorded('k')) == 1 and eng.lib is real
    _sight_at(rp, eng, body, (A, B))
    assert body.calls == 3 and [r[0] for r in ran] == [[A, B]]
    _sight_at(rp, eng, body, (D, D))                         # ... and coinciding inputs never reach a recorded list
    assert body.calls == 4 and body.libs[3] is real and len(ran) == 1
    _sight_at(rp, eng, body, (C, D))
    assert body.calls == 4 and [r[0] for r in ran] == [[A, B], [C, D]]


def test_on_break_reaches_the_replay(built, ran):
    eng, rp, body = _moving(built._lib)
    hook = lambda tag: None
    for _ in range(3):
        _sight_at(rp, eng, body, (A, B), on_break=hook)
    _sight_at(rp, eng, body, (A, B))
    assert [r[1] for r in ran] == [hook, None]
    rp.begin(eng, 'static')(0, body)                         # (inputs=None: nothing moves)
    rp.begin(eng, 'static')(0, body)
    rp.begin(eng, 'static')(0, body, on_break=hook)
    assert ran[-1] == ([A, B], hook)


@pytest.mark.parametrize('lru', [False, True])
def test_clear_empties_keys_and_recorded(built, ran, lru):
    eng, rp, body = _moving(built._lib, lru=lru)
    for key in ('k', 'm'):
        for _ in range(2):
            _sight_at(rp, eng, body, (A, B), key=key)
    assert rp.keys() == ['k', 'm'] and len(rp.recorded()) == 2
    rp.clear()
    assert rp.keys() == [] and rp.recorded() == [] and rp.recorded('k') == []
    _sight_at(rp, eng, body, (A, B))                         # a cleared key is at its first sighting again
    assert body.calls == 5 and body.libs[-1] is eng.lib and rp.recorded() == []
