"""Header chain context — ``hkv_connect_headers*`` and ``hkv_chain_context_device``:
a peer's ``headers`` message in, the answer of haskoin-core ``connectBlocks``
out (``importHeaders``, reference ``src/Haskoin/Node/Chain.hs:500-520``): how many
leading headers connect, and per header the median time past, the expected
bits, the accumulated chain work and the HKV_CHN_* flags. All computation runs
in libhkv's HIP kernels (csrc/hkv_headers.hip, csrc/hkv_chainctx.hip); the rule
is stated in include/hkv.h.

    tip = ChainTip.genesis(params, genesis_header)
    r = connect_headers(v, headers, tip, params, checkpoints=(), now=...)
        -> ConnectResult(hashes, hdr_status, chain_status, mtp, bits, work, n_ok)
    tip = tip.advance(headers, r, r.n_ok)      # the next message's context
"""
from __future__ import annotations

import ctypes
import time as _time
from dataclasses import dataclass, replace
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .headers import HEADER_SIZE
from .lib import (HKV_CHAIN_MIN_DIFFICULTY, HKV_CHAIN_NO_RETARGET, HKV_CHN_ALL, HKV_CHN_BITS_OK,  # noqa: F401
                  HKV_CHN_CHECKPOINT_OK, HKV_CHN_NOT_FUTURE, HKV_CHN_TIME_OK, HKV_CHN_VERSION_OK, HKV_HDR_LINK_OK,
                  HKV_HDR_POW_OK, HkvChainCtx, check)

MTP_SPAN = 11


@dataclass(frozen=True)
class ChainParams:
    """A network's header-chain constants (haskoin-core Haskoin.Network.Constants [dep])."""
    pow_limit: int
    bip34_height: int
    bip66_height: int
    bip65_height: int
    flags: int = 0
    interval: int = 2016
    target_timespan: int = 14 * 24 * 60 * 60
    min_diff_spacing: int = 2 * 10 * 60

    @property
    def limit_bits(self) -> int:
        return encode_compact(self.pow_limit)


PARAMS = {
    "btc": ChainParams(pow_limit=(1 << 224) - 1, bip34_height=227931, bip66_height=363725, bip65_height=388381),
    "btcTest": ChainParams(pow_limit=(1 << 224) - 1, bip34_height=21111, bip66_height=330776, bip65_height=581885,
                           flags=HKV_CHAIN_MIN_DIFFICULTY),
    "btcRegTest": ChainParams(pow_limit=(1 << 255) - 1, bip34_height=100000000, bip66_height=1251, bip65_height=1351,
                              flags=HKV_CHAIN_NO_RETARGET | HKV_CHAIN_MIN_DIFFICULTY),
}


def encode_compact(value: int) -> int:
    """Bitcoin's GetCompact of a non-negative number."""
    size = (value.bit_length() + 7) // 8
    word = value << (8 * (3 - size)) if size <= 3 else value >> (8 * (size - 3))
    if word & 0x00800000:
        word >>= 8
        size += 1
    return (size << 24) | word


def _fields(h: bytes) -> Tuple[int, int, int]:
    """(version, time, bits) of an 80-byte header."""
    return (int.from_bytes(h[0:4], "little"), int.from_bytes(h[68:72], "little"), int.from_bytes(h[72:76], "little"))


@dataclass(frozen=True)
class ConnectResult:
    hashes: List[bytes]
    hdr_status: np.ndarray      # HKV_HDR_* per header
    chain_status: np.ndarray    # HKV_CHN_* per header
    mtp: np.ndarray
    bits: np.ndarray            # the expected bits of every header
    work: List[int]             # the chain work up to and including every header
    n_ok: int                   # leading headers that connect
    params: ChainParams


@dataclass(frozen=True)
class ChainTip:
    """What the next header stands on: the context of one connect_headers call."""
    height: int                 # the tip's height: the next header has height + 1
    times: Tuple[int, ...]      # the last 1..11 timestamps, oldest first, the tip's last
    bits: int
    period_first_time: int      # time of the block at height - (height mod interval)
    period_real_bits: int       # the minimum-difficulty walk's answer at the tip
    work: int

    @classmethod
    def genesis(cls, params: ChainParams, header: bytes, work: Optional[int] = None) -> "ChainTip":
        _, t, bits = _fields(header)
        if work is None:
            work = header_work(bits)
        return cls(0, (t,), bits, t, bits, work)

    def advance(self, headers: Sequence[bytes], result: ConnectResult, n: int) -> "ChainTip":
        """The tip after the first n headers of the batch `result` judged."""
        if n == 0:
            return self
        p = result.params
        f = [_fields(h) for h in headers[:n]]
        height = self.height + n
        start = height - height % p.interval
        first_time = f[start - self.height - 1][1] if start > self.height else self.period_first_time
        real = self.period_real_bits
        for j in range(n - 1, -1, -1):
            if (self.height + 1 + j) % p.interval == 0 or f[j][2] != p.limit_bits:
                real = f[j][2]
                break
        return replace(self, height=height, times=(self.times + tuple(x[1] for x in f))[-MTP_SPAN:], bits=f[-1][2],
                       period_first_time=first_time, period_real_bits=real, work=result.work[n - 1])


def header_work(bits: int) -> int:
    """floor(2^256 / (target + 1)); 0 for a negative, overflowing or zero compact."""
    size, word = bits >> 24, bits & 0x007FFFFF
    if size <= 3:
        word >>= 8 * (3 - size)
    if word == 0 or bits & 0x00800000:
        return 0
    if size > 34 or (word > 0xFF and size > 33) or (word > 0xFFFF and size > 32):
        return 0
    target = word if size <= 3 else word << (8 * (size - 3))
    return (1 << 256) // (target + 1)


def chain_ctx(tip: ChainTip, params: ChainParams, now: int) -> HkvChainCtx:
    """struct hkv_chain_ctx of a tip (ValueError for values the struct cannot hold)."""
    if not 1 <= len(tip.times) <= MTP_SPAN:
        raise ValueError("a tip carries 1..11 timestamps")
    c = HkvChainCtx()
    c.height0 = tip.height + 1
    c.n_prev_times = len(tip.times)
    for j, t in enumerate(tip.times):
        c.prev_times[j] = t
    c.parent_bits = tip.bits
    c.period_first_time = tip.period_first_time
    c.period_real_bits = tip.period_real_bits
    c.parent_work[:] = list((tip.work % (1 << 256)).to_bytes(32, "little"))
    c.now = now
    c.pow_limit[:] = list(params.pow_limit.to_bytes(32, "little"))
    c.interval = params.interval
    c.target_timespan = params.target_timespan
    c.min_diff_spacing = params.min_diff_spacing
    c.bip34_height = params.bip34_height
    c.bip66_height = params.bip66_height
    c.bip65_height = params.bip65_height
    c.flags = params.flags
    return c


def pack_checkpoints(checkpoints) -> Tuple[np.ndarray, np.ndarray]:
    """[(height, 32-byte hash in digest order)] -> (heights uint32[k], hashes uint8[32 k]), as given."""
    cps = list(checkpoints)
    for _, h in cps:
        if len(h) != 32:
            raise ValueError("a checkpoint hash is 32 bytes")
    heights = np.array([h for h, _ in cps], dtype=np.uint32)
    hashes = np.frombuffer(b"".join(h for _, h in cps), dtype=np.uint8).copy()
    return heights, hashes


def _raw(headers) -> np.ndarray:
    if isinstance(headers, np.ndarray):
        raw = np.ascontiguousarray(headers, dtype=np.uint8).reshape(-1)
    elif isinstance(headers, (bytes, bytearray)):
        raw = np.frombuffer(bytes(headers), dtype=np.uint8)
    else:
        for h in headers:
            if len(h) != HEADER_SIZE:
                raise ValueError("a block header is 80 bytes")
        raw = np.frombuffer(b"".join(headers), dtype=np.uint8)
    if raw.size % HEADER_SIZE:
        raise ValueError("header batch is not a multiple of 80 bytes")
    return raw


def work_ints(work: np.ndarray) -> List[int]:
    """n * 32 little-endian bytes -> Python integers."""
    b = np.ascontiguousarray(work, dtype=np.uint8).tobytes()
    return [int.from_bytes(b[32 * i: 32 * i + 32], "little") for i in range(len(b) // 32)]


def connect_headers(v, headers, tip: ChainTip, params: ChainParams, checkpoints=(), now: Optional[int] = None,
                    prev_hash: Optional[bytes] = None) -> ConnectResult:
    """hkv_connect_headers (host memory, first device, blocking). prev_hash:
    the tip's hash in digest order, or None (header 0 then counts as linked)."""
    raw = _raw(headers)
    n = raw.size // HEADER_SIZE
    if prev_hash is not None and len(prev_hash) != 32:
        raise ValueError("prev_hash is 32 bytes")
    ctx = chain_ctx(tip, params, int(_time.time()) if now is None else now)
    cph, cpx = pack_checkpoints(checkpoints)
    hashes = np.zeros(n * 32, dtype=np.uint8)
    hst = np.zeros(n, dtype=np.uint8)
    mtp = np.zeros(n, dtype=np.uint32)
    bits = np.zeros(n, dtype=np.uint32)
    work = np.zeros(n * 32, dtype=np.uint8)
    cst = np.zeros(n, dtype=np.uint8)
    n_ok = ctypes.c_size_t(0)
    prev = None if prev_hash is None else np.frombuffer(prev_hash, dtype=np.uint8).copy()
    rc = v.lib.hkv_connect_headers(v.ctx, raw.ctypes.data, n, None if prev is None else prev.ctypes.data,
                                   ctypes.byref(ctx), cph.ctypes.data if len(cph) else None,
                                   cpx.ctypes.data if len(cph) else None, len(cph), hashes.ctypes.data,
                                   hst.ctypes.data, mtp.ctypes.data, bits.ctypes.data, work.ctypes.data,
                                   cst.ctypes.data, ctypes.byref(n_ok))
    check(rc, "hkv_connect_headers", v.lib)
    hb = hashes.tobytes()
    return ConnectResult([hb[32 * i: 32 * i + 32] for i in range(n)], hst, cst, mtp, bits, work_ints(work),
                         int(n_ok.value), params)


def chain_scratch_words(v, n: int) -> int:
    """hkv_chain_scratch_words: the stage's scratch for n headers, in 32-bit words."""
    return int(v.lib.hkv_chain_scratch_words(n))


def debug_chain_stages(v, dev: int, stages: int) -> None:
    """hkv_debug_chain_stages (measurement hook): the launches later chain-context
    calls run (bit 0 facts, 1 tile scan, 2 verdicts, 3 first_bad)."""
    check(v.lib.hkv_debug_chain_stages(v.ctx, dev, stages & 0xFFFFFFFF), "hkv_debug_chain_stages", v.lib)


def _p(x: Optional[int]):
    return ctypes.c_void_p(x) if x else None


def chain_context_device(v, dev: int, d_headers: int, n: int, d_hashes: Optional[int], ctx: HkvChainCtx,
                         d_cp_heights: Optional[int], d_cp_hashes: Optional[int], n_cp: int, d_mtp: int, d_bits: int,
                         d_work: int, d_status: int, d_scratch: int, stream: int = 0) -> None:
    """hkv_chain_context_device: the stage alone, after check_headers_device on
    the same stream. Enqueued, not synchronised."""
    rc = v.lib.hkv_chain_context_device(v.ctx, dev, _p(d_headers), n, _p(d_hashes), ctypes.byref(ctx),
                                        _p(d_cp_heights), _p(d_cp_hashes), n_cp, _p(d_mtp), _p(d_bits), _p(d_work),
                                        _p(d_status), _p(d_scratch), _p(stream))
    check(rc, "hkv_chain_context_device", v.lib)


def connect_headers_device(v, dev: int, d_headers: int, n: int, d_pow_limit: int, d_prev_hash: Optional[int],
                           ctx: HkvChainCtx, d_cp_heights: Optional[int], d_cp_hashes: Optional[int], n_cp: int,
                           d_hashes: int, d_hdr_status: int, d_mtp: int, d_bits: int, d_work: int, d_status: int,
                           d_scratch: int, d_first_bad: int, stream: int = 0) -> None:
    """hkv_connect_headers_device: the header checks, the stage and the
    first_bad reduction on one stream. Enqueued, not synchronised."""
    rc = v.lib.hkv_connect_headers_device(v.ctx, dev, _p(d_headers), n, _p(d_pow_limit), _p(d_prev_hash),
                                          ctypes.byref(ctx), _p(d_cp_heights), _p(d_cp_hashes), n_cp, _p(d_hashes),
                                          _p(d_hdr_status), _p(d_mtp), _p(d_bits), _p(d_work), _p(d_status),
                                          _p(d_scratch), _p(d_first_bad), _p(stream))
    check(rc, "hkv_connect_headers_device", v.lib)


__all__ = ["ChainParams", "ChainTip", "ConnectResult", "PARAMS", "connect_headers", "connect_headers_device",
           "chain_context_device", "chain_scratch_words", "chain_ctx", "pack_checkpoints", "debug_chain_stages",
           "header_work", "encode_compact", "work_ints", "HKV_CHN_TIME_OK", "HKV_CHN_NOT_FUTURE", "HKV_CHN_BITS_OK",
           "HKV_CHN_VERSION_OK", "HKV_CHN_CHECKPOINT_OK", "HKV_CHN_ALL", "HKV_CHAIN_NO_RETARGET",
           "HKV_CHAIN_MIN_DIFFICULTY"]
