"""Device buffers for the tests of the encoders' device entry points (test_gpu_device_contract.py), after _device_inflate / _guarded_batch of the
reader tests: an input tensor that ends at the input's last byte, an output tensor with guard bytes on both sides of the `cap` bytes the call may
write, and the comparison of the guards, which is plain numpy and has a CPU test of its own (test_guard_comparison_sees_every_edge)."""
import ctypes

import numpy as np

GUARD = 0xA5
TAIL = 48          # the output tensor is a_out + cap + (TAIL - a_out) bytes: at least 32 guard bytes behind cap at every alignment


def guard_damage(buf, a_out, cap, fill=GUARD):
    """Offsets in `buf` (numpy uint8: a_out guard bytes, cap bytes of output, guard bytes to the end) of the guard bytes that are no longer `fill`."""
    buf = np.asarray(buf, dtype=np.uint8)
    assert 0 <= a_out and a_out + cap <= len(buf)
    front = np.flatnonzero(buf[:a_out] != fill)
    back = np.flatnonzero(buf[a_out + cap:] != fill) + (a_out + cap)
    return [int(x) for x in front] + [int(x) for x in back]


def device_call(fn, data, cap, a_in=0, a_out=0):
    """fn (d_in, n, d_out, cap) with the n bytes of `data` at offset a_in of a tensor of a_in + n bytes and the output at offset a_out of a tensor
    of cap + TAIL bytes of GUARD.  Asserts that no guard byte and no byte of the input tensor changed.  -> (what fn returned, the cap output bytes)"""
    import torch
    n = len(data)
    h_in = np.full(max(a_in + n, 1), 0x3C, dtype=np.uint8)           # (an empty tensor has no address: one byte for n = 0 at a_in = 0)
    h_in[a_in:a_in + n] = np.frombuffer(data, dtype=np.uint8)
    t_in = torch.from_numpy(h_in).cuda()
    t_out = torch.full((cap + TAIL,), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    res = fn(t_in.data_ptr() + a_in, n, t_out.data_ptr() + a_out, cap)
    torch.cuda.synchronize()
    host = t_out.cpu().numpy()
    bad = guard_damage(host, a_out, cap)
    assert not bad, "bytes outside the output buffer were written: offsets %r relative to d_out, cap %d" % ([b - a_out for b in bad[:8]], cap)
    assert np.array_equal(t_in.cpu().numpy(), h_in), "the encoder wrote to its input"
    return res, host[a_out:a_out + cap].tobytes()


def guarded_batch(fn, datas, caps, guard=16):
    """fn (count, in pointers, lengths, out pointers, caps, out_len, crc, rc) -- a zada_*_batch of the C ABI with its context and method bound -- on a
    numpy arena with `guard` bytes of GUARD on both sides of every output.  Asserts the guards.  -> (return value, rcs, out_lens, crcs, the cap
    bytes of every output)"""
    cnt = len(datas)
    lens = np.array([len(d) for d in datas], dtype=np.uint64)
    caps = np.array(caps, dtype=np.uint64)
    keep = [bytes(d) if len(d) else b"\0" for d in datas]
    ins = np.array([ctypes.cast(ctypes.c_char_p(d), ctypes.c_void_p).value for d in keep], dtype=np.uint64)
    offs = (np.concatenate(([0], np.cumsum(caps + np.uint64(guard))[:-1])) + guard).astype(np.uint64)
    arena = np.full(int((caps + np.uint64(guard)).sum()) + guard, GUARD, dtype=np.uint8)
    outp = (arena.ctypes.data + offs).astype(np.uint64)
    ols = np.zeros(cnt, np.uint64)
    crcs = np.full(cnt, 0xFFFFFFFF, dtype=np.uint32)
    rcs = np.full(cnt, 99, dtype=np.int32)
    worst = fn(cnt, ins.ctypes.data, lens.ctypes.data, outp.ctypes.data, caps.ctypes.data, ols.ctypes.data, crcs.ctypes.data, rcs.ctypes.data)
    outs = []
    for k in range(cnt):
        o, cap = int(offs[k]), int(caps[k])
        bad = guard_damage(arena[o - guard:o + cap + guard], guard, cap)
        assert not bad, "entry %d: bytes outside its output buffer were written: offsets %r relative to out, cap %d" % (k, [b - guard for b in bad[:8]], cap)
        outs.append(arena[o:o + cap].tobytes())
    return worst, rcs, ols, crcs, outs
