"""Scan and stable radix sort of the binning stage, through the C ABI test hooks: bit-exact vs torch."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def _lib():
    import diff_gaussian_rasterization as D
    assert torch.cuda.is_available()
    return D._load(), D


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("n", [1, 63, 64, 4095, 4096, 4097, 100_000, 1_234_567, 20_000_001])
def test_exclusive_scan(n):
    lib, D = _lib()
    g = torch.Generator().manual_seed(n)
    x = torch.randint(0, 1000, (n,), generator=g, dtype=torch.int32).cuda()
    out = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    rc = lib.gsr_test_scan(x.data_ptr(), out.data_ptr(), n, _stream())
    assert rc == 0, D._err(lib)
    ref = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(x.cpu().long(), 0)])
    assert torch.equal(out.cpu().long() & 0xFFFFFFFF, ref & 0xFFFFFFFF)     # 32-bit prefix sums (the 20 M case wraps)


@pytest.mark.parametrize("n,lo,hi", [(1, 0, 32), (1000, 0, 32), (4096, 0, 13), (4097, 0, 8), (300_001, 0, 32),
                                     (2_000_003, 0, 13), (50_000, 0, 15), (70_000, 3, 9)])
def test_stable_radix_sort_pairs(n, lo, hi):
    lib, D = _lib()
    g = torch.Generator().manual_seed(n + hi)
    # few distinct keys => many ties => stability is exercised
    keys = torch.randint(0, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64)
    if hi - lo < 32:
        keys = keys % (1 << min(hi, 20))
    keys32 = keys.to(torch.int32).cuda()
    vals = torch.randint(0, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int32).cuda()
    k, v = keys32.clone(), vals.clone()
    rc = lib.gsr_test_sort_pairs(k.data_ptr(), v.data_ptr(), n, lo, hi, 0, _stream())
    assert rc == 0, D._err(lib)
    digit = (keys >> lo) & ((1 << (hi - lo)) - 1)
    order = torch.argsort(digit, stable=True)
    assert torch.equal(k.cpu().long(), keys[order])
    assert torch.equal(v.cpu(), vals.cpu()[order])
    # argsort form (iota): vals are the permutation
    k2, v2 = keys32.clone(), torch.empty_like(vals)
    rc = lib.gsr_test_sort_pairs(k2.data_ptr(), v2.data_ptr(), n, lo, hi, 1, _stream())
    assert rc == 0, D._err(lib)
    assert torch.equal(v2.cpu().long(), order)


def test_float_depth_keys_sort_like_floats():
    lib, D = _lib()
    n = 200_000
    d = (torch.rand(n, generator=torch.Generator().manual_seed(5)) * 100 + 0.2).float()
    d[::7] = d[3]            # ties
    k = d.view(torch.int32).cuda()
    v = torch.empty(n, dtype=torch.int32, device="cuda")
    assert lib.gsr_test_sort_pairs(k.data_ptr(), v.data_ptr(), n, 0, 32, 1, _stream()) == 0
    assert torch.equal(v.cpu().long(), torch.argsort(d, stable=True))


# ---- the same primitives with every argument the forward uses (gsr_test_scan_ex / gsr_test_sort_pairs_ex) ----------
SENT = 0x5A5A5A5A                                              # what the tests pre-fill words with that must stay untouched
EMPTY_RANGE = (0xFFFFFFFF, 0)
SCAN_SIZES = [1, 2047, 2048, 2049, 4097, 2 << 20, (2 << 20) + 1]   # the last two: largest 8-item case, smallest 16-item one


def _i32(t):
    """int64 values in [0, 2^32) as the int32 words the device sees."""
    return torch.where(t >= 2 ** 31, t - 2 ** 32, t).to(torch.int32)


def _u32(t):
    return t.cpu().long() & 0xFFFFFFFF


_SCAN_INPUTS = {}


def _scan_input(n):
    """(values, exclusive prefix sums with the total appended, masked to 32 bits) on the CPU, made once per size."""
    if n not in _SCAN_INPUTS:
        x = torch.randint(0, 1000, (n,), generator=torch.Generator().manual_seed(n), dtype=torch.int64)
        ref = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(x, 0)]) & 0xFFFFFFFF
        _SCAN_INPUTS[n] = (x, ref)
    return _SCAN_INPUTS[n]


def _live_counts(n):
    return sorted({c for c in (0, 1, n - 1, n, n + 5) if c >= 0})


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_with_a_device_live_count(n):
    lib, D = _lib()
    x, ref = _scan_input(n)
    xd = _i32(x).cuda()
    for count in _live_counts(n):
        live = min(count, n)                                   # a live count above n clamps to n
        out = torch.full((n + 8,), SENT, dtype=torch.int32, device="cuda")
        nd = _i32(torch.tensor([count])).cuda()
        rc = lib.gsr_test_scan_ex(xd.data_ptr(), out.data_ptr(), n, nd.data_ptr(), None, 0, 0, _stream())
        assert rc == 0, D._err(lib)
        got = _u32(out)
        assert torch.equal(got[:live + 1], ref[:live + 1]), f"n={n} live={count}"     # out[live] = total of the live part
        assert bool((got[live + 1:] == SENT).all()), f"n={n} live={count}: words behind out[live] were written"
        assert torch.equal(_u32(xd), x)


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_in_place(n):
    lib, D = _lib()
    x, ref = _scan_input(n)
    for count in (None, n - 1):
        live = n if count is None else count
        buf = torch.full((n + 8,), SENT, dtype=torch.int32, device="cuda")
        buf[:n] = _i32(x).cuda()
        nd = None if count is None else _i32(torch.tensor([count])).cuda()
        rc = lib.gsr_test_scan_ex(buf.data_ptr(), buf.data_ptr(), n, None if nd is None else nd.data_ptr(), None, 0, 0, _stream())
        assert rc == 0, D._err(lib)
        got = _u32(buf)
        assert torch.equal(got[:live + 1], ref[:live + 1]), f"n={n} live={count}"
        assert torch.equal(got[live + 1:n], x[live + 1:]) and bool((got[max(n, live + 1):] == SENT).all())


@pytest.mark.parametrize("n", SCAN_SIZES)
@pytest.mark.parametrize("in_off,out_off", [(1, 1), (1, 0), (0, 1)])
def test_scan_one_word_off_a_16_byte_boundary(n, in_off, out_off):
    """Input and / or output start 4 bytes behind a 16-byte boundary: the threads' 16-byte loads / stores are not possible."""
    lib, D = _lib()
    x, ref = _scan_input(n)
    xin = torch.zeros(n + 4, dtype=torch.int32, device="cuda")
    xin[in_off:in_off + n] = _i32(x).cuda()
    out = torch.full((n + 12,), SENT, dtype=torch.int32, device="cuda")
    pin, pout = xin.data_ptr() + 4 * in_off, out.data_ptr() + 4 * out_off
    assert xin.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    rc = lib.gsr_test_scan_ex(pin, pout, n, None, None, 0, 0, _stream())
    assert rc == 0, D._err(lib)
    got = _u32(out)
    assert torch.equal(got[out_off:out_off + n + 1], ref)
    assert bool((got[:out_off] == SENT).all()) and bool((got[out_off + n + 1:] == SENT).all())


def _run_lengths(n, seed, chunk_len):
    """Run lengths for chunk_first: runs of zeros (five at the very start), mostly 0..3, one in 300 larger than two chunks (one
    element then owns several chunk starts), and a total that is an exact multiple of chunk_len."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 4, (n,), generator=g, dtype=torch.int64) * (torch.rand(n, generator=g) < 0.3)
    if n > 40:
        x[:5] = 0
        x[n // 3:n // 3 + 30] = 0
        big = torch.randperm(n - 10, generator=g)[:max(n // 300, 2)] + 5
        x[big] = torch.randint(2 * chunk_len + 1, 9 * chunk_len, (big.numel(),), generator=g, dtype=torch.int64)
    x[n // 2] += (-int(x.sum())) % chunk_len
    if int(x.sum()) == 0:
        x[n // 2] = chunk_len
    assert int(x.sum()) % chunk_len == 0 and 0 < int(x.sum()) < 2 ** 32
    return x


@pytest.mark.parametrize("n", [1, 7, 2049, 10_001, (2 << 20) + 1])
def test_scan_chunk_first(n):
    """chunk_first[c] = the element r with out[r] <= c * chunk_len < out[r] + in[r], for every c < chunk_cap whose c * chunk_len
    is below the total (of the live part); every other entry keeps its sentinel."""
    lib, D = _lib()
    L = 2048
    x = _run_lengths(n, n + 1, L)
    xd = _i32(x).cuda()
    for count in (None, n - n // 3):
        live = n if count is None else count
        incl = torch.cumsum(x[:live], 0)
        total = int(incl[-1]) if live else 0
        ref = torch.cat([torch.zeros(1, dtype=torch.int64), incl])
        nstarts = (total + L - 1) // L                          # chunk starts c * L below the total
        owner = torch.searchsorted(incl, torch.arange(nstarts, dtype=torch.int64) * L, right=True)   # first r: incl[r] > c L
        if count is None:
            assert total % L == 0 and nstarts == total // L     # the entry of c = total / L itself stays untouched
        for cap in sorted({nstarts + 3, nstarts, nstarts // 2, 0}):
            out = torch.full((n + 8,), SENT, dtype=torch.int32, device="cuda")
            cf = torch.full((nstarts + 8,), SENT, dtype=torch.int32, device="cuda")
            nd = None if count is None else _i32(torch.tensor([count])).cuda()
            rc = lib.gsr_test_scan_ex(xd.data_ptr(), out.data_ptr(), n, None if nd is None else nd.data_ptr(), cf.data_ptr(), L, cap,
                                      _stream())
            assert rc == 0, D._err(lib)
            got, gcf = _u32(out), _u32(cf)
            assert torch.equal(got[:live + 1], ref) and bool((got[live + 1:] == SENT).all())
            k = min(cap, nstarts)
            assert torch.equal(gcf[:k], owner[:k]), f"n={n} live={count} cap={cap}"
            assert bool((gcf[k:] == SENT).all()), f"n={n} live={count} cap={cap}: entries beyond the chunk starts / the cap were written"
    assert int((x > 2 * L).sum()) > 0 or n < 40


SORT_BITS = [(0, 32), (0, 13), (3, 9)]
_SORT_INPUTS = {}


def _sort_input(n):
    """(keys, vals) on the CPU as int64 in [0, 2^32): keys drawn from 48 values (0 and 2^32 - 1 among them), so that every
    digit has long runs of ties whose keys differ outside the digit -- stability decides keys and values alike."""
    if n not in _SORT_INPUTS:
        g = torch.Generator().manual_seed(n)
        palette = torch.randint(0, 2 ** 32, (48,), generator=g, dtype=torch.int64)
        palette[0], palette[1] = 0, 2 ** 32 - 1
        keys = palette[torch.randint(0, 48, (n,), generator=g)]
        vals = torch.randint(0, 2 ** 32, (n,), generator=g, dtype=torch.int64)
        _SORT_INPUTS[n] = (keys, vals)
    return _SORT_INPUTS[n]


def _check_sort(lib, D, n, lo, hi, rounds, live_count=None):
    keys, vals = _sort_input(n)
    live = n if live_count is None else min(live_count, n)
    digit = (keys[:live] >> lo) & ((1 << (hi - lo)) - 1)
    order = torch.argsort(digit, stable=True)
    nd = None if live_count is None else _i32(torch.tensor([live_count])).cuda()
    ndp = None if nd is None else nd.data_ptr()
    k, v = _i32(keys).cuda(), _i32(vals).cuda()
    rc = lib.gsr_test_sort_pairs_ex(k.data_ptr(), v.data_ptr(), n, ndp, lo, hi, 0, rounds, None, 0, _stream())
    assert rc == 0, D._err(lib)
    assert torch.equal(_u32(k)[:live], keys[:live][order]), "pair form: keys"
    assert torch.equal(_u32(v)[:live], vals[:live][order]), "pair form: values"
    k2, v2 = _i32(keys).cuda(), torch.full((n,), SENT, dtype=torch.int32, device="cuda")
    rc = lib.gsr_test_sort_pairs_ex(k2.data_ptr(), v2.data_ptr(), n, ndp, lo, hi, 1, rounds, None, 0, _stream())
    assert rc == 0, D._err(lib)
    assert torch.equal(_u32(v2)[:live], order), "iota form: the permutation"
    assert torch.equal(_u32(k2)[:live], keys[:live][order]), "iota form: keys"


@pytest.mark.parametrize("lo,hi", SORT_BITS)
@pytest.mark.parametrize("edge", ["1", "chunk-1", "chunk", "chunk+1", "3chunk+1"])
@pytest.mark.parametrize("rounds", [8, 16])
def test_sort_at_the_chunk_edges(rounds, edge, lo, hi):
    lib, D = _lib()
    chunk = 256 * rounds
    n = {"1": 1, "chunk-1": chunk - 1, "chunk": chunk, "chunk+1": chunk + 1, "3chunk+1": 3 * chunk + 1}[edge]
    _check_sort(lib, D, n, lo, hi, rounds)


@pytest.mark.parametrize("lo,hi", SORT_BITS)
@pytest.mark.parametrize("rounds", [8, 16])
def test_sort_with_digit_rows_longer_than_one_rowscan_batch(rounds, lo, hi):
    """514 blocks: a digit's row of per-block counts takes two 512-word batches of k_radix_rowscan."""
    lib, D = _lib()
    _check_sort(lib, D, 513 * 256 * rounds + 1, lo, hi, rounds)


@pytest.mark.parametrize("lo,hi", [(0, 32), (0, 13)])
@pytest.mark.parametrize("rounds", [8, 16])
def test_sort_with_a_device_live_count(rounds, lo, hi):
    """Only positions below the live count are sorted and compared."""
    lib, D = _lib()
    chunk = 256 * rounds
    n = 3 * chunk + 1
    for count in (0, 1, chunk, n - 1):
        _check_sort(lib, D, n, lo, hi, rounds, live_count=count)


@pytest.mark.parametrize("T,nchunks", [(1, 1), (1, 5), (5, 5), (1000, 5), (1000, 1)])
@pytest.mark.parametrize("rounds", [8, 16])
def test_sort_leaves_the_key_ranges(rounds, T, nchunks):
    """Keys 0..T as the tile sort sees them (T = the key of a culled pair, which gets no range): after the sort every present key
    below T has [first, last + 1) of its run, every absent one keeps (0xFFFFFFFF, 0).  One key takes half of the elements, so
    with five chunks its run spreads over several blocks."""
    lib, D = _lib()
    n = nchunks * 256 * rounds + 3
    g = torch.Generator().manual_seed(1000 * T + n)
    mask = torch.rand(T, generator=g) < 0.6
    mask[T // 2], mask[T - 1] = False, True                    # some keys absent, some present
    present = torch.nonzero(mask).flatten()
    if T == 1:
        present = torch.zeros(1 if nchunks == 5 else 0, dtype=torch.int64)    # key 0 present / only culled pairs
    pool = torch.cat([present, torch.tensor([T])])
    keys = pool[torch.randint(0, pool.numel(), (n,), generator=g)]
    keys[torch.rand(n, generator=g) < 0.5] = pool[0]
    vals = torch.arange(n, dtype=torch.int64)
    end_bit = T.bit_length()
    k, v = _i32(keys).cuda(), _i32(vals).cuda()
    kr = torch.full((2 * T + 2,), SENT, dtype=torch.int32, device="cuda")
    kr[:2 * T] = _i32(torch.tensor(EMPTY_RANGE).repeat(T)).cuda()
    rc = lib.gsr_test_sort_pairs_ex(k.data_ptr(), v.data_ptr(), n, None, 0, end_bit, 0, rounds, kr.data_ptr(), T, _stream())
    assert rc == 0, D._err(lib)
    order = torch.argsort(keys, stable=True)
    skeys = keys[order]
    assert torch.equal(_u32(k), skeys) and torch.equal(_u32(v), vals[order])
    ids = torch.arange(T, dtype=torch.int64)
    first, end = torch.searchsorted(skeys, ids, right=False), torch.searchsorted(skeys, ids, right=True)
    there = end > first
    assert torch.equal(torch.nonzero(there).flatten(), present[torch.isin(present, keys)])
    want = torch.stack([torch.where(there, first, torch.tensor(EMPTY_RANGE[0])), torch.where(there, end, torch.tensor(EMPTY_RANGE[1]))], 1)
    got = _u32(kr)
    assert torch.equal(got[:2 * T].view(T, 2), want)
    assert bool((got[2 * T:] == SENT).all())                   # the culled key leaves no range
    if nchunks == 5 and pool[0] < T:
        assert int(end[pool[0]] - first[pool[0]]) > 2 * 256 * rounds
