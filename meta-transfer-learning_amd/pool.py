"""Buffer pool of a pass engine: named buffers of the current pass (the arena) over a bounded pool of allocations, the byte budget
the pools of one device share, and the scratch buffer of the main stream.  Nothing here calls the library or needs a device:
PassEngine derives from BufferPool, and tests/test_pool.py runs the policy on the CPU.

Real manifests bring a new (T, Td) with almost every batch (collate pads to the batch maximum; padding further would change
results: the reference masks with RAW frame counts).  The pool is therefore bounded: entries carry the number of the last
pass that touched them, and trim_pool() -- start of every forward -- drops the least recently used ones that neither this pass nor
the previous one uses while the pools of ALL engines on this device (a model has one per task lane) together hold more than
MTL_POOL_GB (default: a quarter of the device's memory, 72 GiB of the 288; a budget per engine let eight lanes keep 8 x 48 GiB of
stale shapes and ran a north-star run on ragged batches out of memory).  An eviction bumps scratch_epoch, which makes the trainer
re-record its command lists (they hold raw addresses).
"""
import os
import re
import weakref

import torch

LAYER_BUF = re.compile(r'^([de])(\d+)\.(.+)$')      # 'd3.sa.q': a buffer of decoder layer 3

_POOL_ACCOUNTS = {}


def new_account(budget):
    """bytes held by a set of pools, the budget they share, their pass count and (weakly) the pools themselves"""
    return dict(bytes=0, budget=int(budget), gen=0, engines=[])


def _pool_account(device):
    """Bytes held by the buffer pools of every engine on one device, and the budget they share (MTL_POOL_GB)."""
    key = (device.type, device.index)
    acc = _POOL_ACCOUNTS.get(key)
    if acc is None:
        gb = os.environ.get('MTL_POOL_GB')
        if gb is not None:
            budget = int(float(gb) * (1 << 30))
        elif device.type == 'cuda':
            budget = max(torch.cuda.get_device_properties(device).total_memory // 4, 4 << 30)
        else:
            budget = 4 << 30
        acc = _POOL_ACCOUNTS[key] = new_account(budget)
    return acc


class BufferPool:
    def __init__(self, device, layer_slots, account=None):
        """layer_slots: {'d': decoder layers, 'e': encoder layers} -- the slots of a per-layer buffer group (buf);
        account: the one of `device` unless given (new_account: tests keep theirs apart)"""
        self.device = device
        self.layer_slots = layer_slots
        self.arena = {}     # name -> buffer of the current pass (looked up again by the backward)
        self.pool = {}      # (name, shape, dtype) -> allocation, so alternating batch shapes do not re-allocate
        self.account = _pool_account(device) if account is None else account
        self.account['engines'] = [w for w in self.account['engines'] if w() is not None] + [weakref.ref(self)]
        self._last_pass = self.account['gen']       # the account's pass count at this pool's latest pass (trim_pool)
        self.pool_budget = self.account['budget']           # (a pool may be given a tighter one of its own: tests)
        self._pool_gen, self._pool_bytes, self._gen = {}, 0, 0
        self.scratch_epoch = 0

    def _took(self, nbytes):
        self._pool_bytes += nbytes
        self.account['bytes'] += nbytes

    def __del__(self):
        try:
            self.account['bytes'] -= self._pool_bytes     # the device-wide account outlives the engine
        except Exception:
            pass

    def _alloc(self, key):
        t = torch.empty(key[1], dtype=key[2], device=self.device)
        self.pool[key] = t
        self._took(t.numel() * t.element_size())
        return t

    def buf(self, name, shape, dtype=torch.float32):
        """Named buffer of the current pass.  Per-layer buffers ('d<i>.<what>', 'e<i>.<what>') are slices of ONE allocation per
        <what> with the layers at a constant stride -- 'dec_in.y' / 'enc_in.y' are slot 0 of the '<x>.ff.y' group, so that every
        layer's INPUT is at that stride too -- which lets the weight-gradient products of all layers of a stack run as one
        strided-batch launch (PassEngine.flush_layer_wgrads)."""
        shape = tuple(int(v) for v in shape)
        m = LAYER_BUF.match(name)
        if m or name in ('dec_in.y', 'enc_in.y'):
            kind, idx, rest = (m.group(1), int(m.group(2)), m.group(3)) if m else (name[0], -1, 'ff.y')
            n = self.layer_slots[kind] + (1 if rest == 'ff.y' else 0)
            slot = idx + 1 if rest == 'ff.y' else idx
            if 0 <= slot < n:
                key = (kind + '*.' + rest, (n,) + shape, dtype)
                grp = self.pool.get(key)
                if grp is None:
                    grp = self._alloc(key)
                self._pool_gen[key] = self._gen
                t = grp[slot]
                self.arena[name] = t
                return t
        key = (name, shape, dtype)
        t = self.pool.get(key)
        if t is None:
            t = self._alloc(key)
        self._pool_gen[key] = self._gen
        self.arena[name] = t
        return t

    def _over(self):
        return self._pool_bytes > self.pool_budget or self.account['bytes'] > self.account['budget']

    def _pool_invalidated(self):
        """an eviction freed buffers: the owner drops what it keyed by their addresses"""

    def _evict(self, evictable):
        """drop the least recently used pool entries `evictable(key)` accepts while the pool / the device-wide account is over its
        budget; -> bytes freed.  An eviction invalidates everything that holds addresses (tables, arena, recorded command lists)."""
        freed = 0
        for key in sorted(self.pool, key=lambda k: self._pool_gen.get(k, 0)):
            if not self._over() or not evictable(key):
                break
            t = self.pool.pop(key)
            self._pool_gen.pop(key, None)
            nb = t.numel() * t.element_size()
            self._took(-nb)
            freed += nb
        if freed:
            self._pool_invalidated()
            self.arena = {k: v for k, v in self.arena.items() if not isinstance(v, torch.Tensor) or k == '_scratch'}
            self.scratch_epoch += 1
        return freed

    def trim_pool(self):
        """Start of a pass: count it, and while the pool is over its budget drop least-recently-used buffers that the last two
        passes did not touch (a forward and its backward, and the pass a pipelined host has already enqueued, keep theirs).
        The budget is shared by all engines of the device (a model has one per task lane), and an engine can only give up its OWN
        buffers during its own pass: when the shared account is over, the engines that have been IDLE for a while (no pass among the
        device's last max(8, 4 x engines) passes: lanes a changed schedule no longer uses) are emptied first -- otherwise the one
        engine doing the work would stay over budget for ever, dropping and re-allocating its own shapes (and re-recording the
        trainer's command lists) on every pass.
        Frees go back to torch's caching allocator in stream order: the side stream was joined at the end of the backward, and a
        block returns to the free list of the stream it was allocated on."""
        self._gen += 1
        acc = self.account
        acc['gen'] += 1
        self._last_pass = acc['gen']
        if not self._over():
            return 0
        if self.device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
            return 0                      # a free inside a hipGraph capture would be baked into the graph: trim at the next eager pass
        freed = 0
        if acc['bytes'] > acc['budget']:
            others = [e for e in (w() for w in acc['engines']) if e is not None and e is not self]
            idle_after = max(8, 4 * (len(others) + 1))
            for e in sorted(others, key=lambda e_: e_._last_pass):
                if acc['bytes'] <= acc['budget'] or acc['gen'] - e._last_pass < idle_after:
                    break
                freed += e._evict(lambda key: True)
        if self._over():
            freed += self._evict(lambda key: self._pool_gen.get(key, 0) < self._gen - 2)
        return freed

    def scratch(self, nbytes):
        """address of the main stream's scratch buffer, grown when `nbytes` do not fit"""
        t = self.arena.get('_scratch')
        if t is None or t.numel() * 4 < nbytes:
            t = torch.empty((int(nbytes) + 3) // 4 + 1024, dtype=torch.float32, device=self.device)
            self.arena['_scratch'] = t
            self.scratch_epoch += 1          # recorded command lists hold the old address: their keys start over (_lib.Replay)
        return t.data_ptr()
