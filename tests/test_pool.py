"""pool.BufferPool on the CPU: layer groups, the two-pass protection and LRU order of trim_pool, the budget several pools share, what an
eviction invalidates, the account's lifetime and the scratch buffer.  The figures are those the same scenarios gave on PassEngine's own
methods before the pool became a module of its own (bound to a stand-in object: PassEngine itself needs a device)."""
import gc

import pytest
import torch

F32 = torch.float32
SLOTS = {'d': 2, 'e': 3}


@pytest.fixture(scope='module')
def P():
    import mtl_amd  # noqa: F401
    from mtl_amd import pool
    return pool


class _Counting:
    """mixed into a pool: counts the invalidation calls"""
    invalidated = 0

    def _pool_invalidated(self):
        self.invalidated += 1


def _make(P, budget=None, account=None, account_budget=1 << 30):
    class Pool(_Counting, P.BufferPool):
        pass
    p = Pool(torch.device('cpu'), SLOTS, P.new_account(account_budget) if account is None else account)
    if budget is not None:
        p.pool_budget = budget
    return p


def _one_pass(p, *names_and_floats):
    freed = p.trim_pool()
    for name, n in names_and_floats:
        p.buf(name, (n,))
    return freed


def test_layers_of_a_stack_are_slices_of_one_allocation(P):
    p = _make(P)
    q0, q2 = p.buf('e0.sa.q', (4, 8)), p.buf('e2.sa.q', (4, 8))
    assert q0.shape == q2.shape == (4, 8) and q2.data_ptr() - q0.data_ptr() == 4 * 64
    assert list(p.pool) == [('e*.sa.q', (3, 4, 8), F32)] and p._pool_bytes == 384 and p.account['bytes'] == 384
    assert p.arena['e0.sa.q'] is q0 and p.arena['e2.sa.q'] is q2
    # the input of layer 0 is slot 0 of the group of the layers' outputs: n_enc + 1 slots
    y = [p.buf(name, (4, 8)) for name in ('enc_in.y', 'e0.ff.y', 'e2.ff.y')]
    assert [t.data_ptr() - y[0].data_ptr() for t in y] == [0, 4 * 32, 4 * 96]
    assert ('e*.ff.y', (4, 4, 8), F32) in p.pool and len(p.pool) == 2
    d = [p.buf(name, (4, 8)) for name in ('dec_in.y', 'd1.ff.y')]
    assert d[1].data_ptr() - d[0].data_ptr() == 4 * 64 and ('d*.ff.y', (3, 4, 8), F32) in p.pool
    # a layer index outside the stack: a plain entry under its own name
    taken = p._pool_bytes
    p.buf('e3.sa.q', (4, 8))
    assert ('e3.sa.q', (4, 8), F32) in p.pool and p._pool_bytes == taken + 128
    # asked again: the same memory, no bytes
    again = p.buf('e0.sa.q', (4, 8))
    assert again.data_ptr() == q0.data_ptr() and p._pool_bytes == taken + 128 and p.account['bytes'] == p._pool_bytes
    # another shape or dtype of the same name is another allocation
    p.buf('e0.sa.q', (4, 8), torch.uint8)
    assert ('e*.sa.q', (3, 4, 8), torch.uint8) in p.pool and p._pool_bytes == taken + 128 + 96


def test_the_last_two_passes_keep_their_buffers_and_the_oldest_goes_first(P):
    p = _make(P, budget=1000)
    assert _one_pass(p, ('a', 100), ('b', 100)) == 0
    assert _one_pass(p, ('c', 100)) == 0                       # (under the budget when the pass begins)
    assert p._pool_bytes == 1200
    assert _one_pass(p, ('c', 100)) == 0                       # over, but a and b are of the pass before the previous one at most
    assert p._pool_bytes == 1200 and p.scratch_epoch == 0 and p.invalidated == 0
    assert _one_pass(p, ('c', 100)) == 400                     # only what the budget needs, the oldest first: a
    assert [k[0] for k in p.pool] == ['b', 'c'] and p._pool_bytes == 800 and p.account['bytes'] == 800
    assert p.scratch_epoch == 1 and p.invalidated == 1
    assert set(p._pool_gen) == set(p.pool)


def test_over_budget_with_nothing_stale_evicts_nothing(P):
    p = _make(P, budget=1000)
    for _ in range(6):
        assert _one_pass(p, ('w1', 200), ('w2', 100)) == 0
    assert p._pool_bytes == 1200 and p.scratch_epoch == 0 and p.invalidated == 0


def test_an_eviction_clears_the_tensors_of_the_arena_but_the_scratch(P):
    p = _make(P, budget=1000)
    _one_pass(p, ('a', 100), ('b', 100))
    p.scratch(64)
    p.arena['note'] = (1, 2)
    epoch = p.scratch_epoch
    for _ in range(3):
        freed = _one_pass(p, ('c', 100))
    assert freed == 400 and p.scratch_epoch == epoch + 1
    # (c was taken after the eviction, in the same pass)
    assert {k for k, v in p.arena.items() if isinstance(v, torch.Tensor)} == {'_scratch', 'c'}
    assert p.arena['note'] == (1, 2)


def test_a_shared_budget_empties_the_idle_pool_first(P):
    acc = P.new_account(3000)
    idle, w = _make(P, account=acc), _make(P, account=acc)
    assert idle.pool_budget == w.pool_budget == 3000 and [r() for r in acc['engines']] == [idle, w]
    _one_pass(idle, ('i', 300), ('j', 200))
    _one_pass(w, ('w1', 200))
    assert acc['bytes'] == 2800
    freed = [_one_pass(w, ('w1', 200), ('w2', 100)) for _ in range(6)]
    assert freed == [0] * 6 and acc['bytes'] == 3200 and acc['gen'] == 8
    # the device's ninth pass; idle's last one was the first: 9 - 1 reaches max(8, 4 x 2 pools)
    assert _one_pass(w, ('w1', 200), ('w2', 100)) == 1200
    assert [k[0] for k in idle.pool] == ['j'] and idle._pool_bytes == 800 and acc['bytes'] == 2000
    assert (idle.scratch_epoch, idle.invalidated) == (1, 1) and (w.scratch_epoch, w.invalidated) == (0, 0)
    assert [k[0] for k in w.pool] == ['w1', 'w2']


def test_a_deleted_pool_gives_its_bytes_back_to_the_account(P):
    acc = P.new_account(1 << 20)
    keep, p = _make(P, account=acc), _make(P, account=acc)
    keep.buf('k', (25,))
    p.buf('x', (1000,))
    assert acc['bytes'] == 4100
    del p
    gc.collect()
    assert acc['bytes'] == 100
    _make(P, account=acc)
    assert [r() for r in acc['engines'][:-1]] == [keep]        # dead pools leave the list when the next one joins


def test_the_device_account_is_one_per_device(P, monkeypatch):
    monkeypatch.setattr(P, '_POOL_ACCOUNTS', {})
    monkeypatch.setenv('MTL_POOL_GB', '0.5')
    a, b = (P.BufferPool(torch.device('cpu'), SLOTS) for _ in range(2))
    assert a.account is b.account and a.account['budget'] == 1 << 29 and a.pool_budget == 1 << 29
    monkeypatch.setattr(P, '_POOL_ACCOUNTS', {})
    monkeypatch.delenv('MTL_POOL_GB')
    assert P.BufferPool(torch.device('cpu'), SLOTS).account['budget'] == 4 << 30


def test_scratch_grows_and_counts_an_epoch_when_it_moves(P):
    p = _make(P)
    first = p.scratch(100)
    assert p.scratch_epoch == 1 and p.arena['_scratch'].numel() * 4 >= 100
    assert p.scratch(50) == first and p.scratch_epoch == 1
    assert p.scratch(10 ** 6) != first and p.scratch_epoch == 2 and p.arena['_scratch'].numel() * 4 >= 10 ** 6
    assert p._pool_bytes == 0                                  # (the scratch is not a pool entry)


def test_side_stream_scratch_is_the_engines_and_is_size_checked(P):
    from mtl_amd.engine import PassEngine

    class Eng(PassEngine):
        def __init__(self):
            P.BufferPool.__init__(self, torch.device('cpu'), SLOTS, P.new_account(1 << 20))
            self.scratch_side, self.on_side, self._ln_tables = torch.empty(16), True, {}

    e = Eng()
    assert e.scratch(64) == e.scratch_side.data_ptr() and e.scratch_epoch == 0 and '_scratch' not in e.arena
    with pytest.raises(RuntimeError, match='side-stream scratch too small'):
        e.scratch(65)
    e.on_side = False
    assert e.scratch(64) == e.arena['_scratch'].data_ptr() != e.scratch_side.data_ptr() and e.scratch_epoch == 1


def test_the_engine_bounds_its_own_tables_after_the_count_of_the_pass(P):
    from mtl_amd.engine import PassEngine

    class Eng(PassEngine):
        def __init__(self):
            P.BufferPool.__init__(self, torch.device('cpu'), SLOTS, P.new_account(1 << 20))
            self._ln_tables = {}

    e = Eng()
    e._ln_tables.update((i, None) for i in range(512))
    assert e.trim_pool() == 0 and len(e._ln_tables) == 512 and e.scratch_epoch == 0 and e._gen == 1
    e._ln_tables[512] = None
    assert e.trim_pool() == 0 and not e._ln_tables and e.scratch_epoch == 1 and e._gen == 2 and e.account['gen'] == 2
    # an eviction clears them through _pool_invalidated
    e.pool_budget = 1000
    e._ln_tables['t'] = None
    _one_pass(e, ('a', 100), ('b', 100))
    for _ in range(3):
        freed = _one_pass(e, ('c', 100))
    assert freed == 400 and not e._ln_tables and e.scratch_epoch == 2
