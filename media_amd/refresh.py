"""Intra refresh on the receiving side: which band a picture refreshes, where a receiver may join, and from which picture on it
has every sample (include/mi355x_h264.h, "intra refresh").  Plain Python on Annex-B bytes and picture counts; no device, no library."""
from .temporal import _nal_spans


def schedule(n, pictures):
    """the all-intra band of pictures 0 .. pictures - 1 of a GOP with n bands: -1 for the IDR picture at position 0, then
    k = (p - 1) mod n for the p-th P picture"""
    if not 2 <= n <= 32:
        raise ValueError("intra refresh: 2 .. 32 bands")
    return [-1 if p == 0 else (p - 1) % n for p in range(pictures)]


def recovered_at(i, n):
    """a receiver whose first good access unit is picture i (position in the GOP, i >= 1 and k(i) = 0: a recovery point) has every
    sample right from this picture on: i + recovery_frame_cnt = i + n - 1.  Band j is right from picture i + j on"""
    if i < 1 or (i - 1) % n != 0:
        raise ValueError("picture %d starts no refresh cycle of %d bands" % (i, n))
    return i + n - 1


def _rbsp(nal_payload):
    out, zeros = bytearray(), 0
    for b in nal_payload:
        if zeros >= 2 and b == 3:
            zeros = 0
            continue
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    return bytes(out)


def _recovery_frame_cnt(rbsp):
    """recovery_frame_cnt of the first recovery point message (payload type 6) of an SEI RBSP, or None - also for an RBSP that
    ends inside a message (bytes from a network: a truncated or foreign SEI is passed over, never an exception)"""
    i, n = 0, len(rbsp)

    def ff_coded(i):   # 7.3.2.3.1: 0xFF bytes, then the last byte; None past the end
        v = 0
        while i < n and rbsp[i] == 0xFF:
            v, i = v + 255, i + 1
        return (None, i) if i >= n else (v + rbsp[i], i + 1)
    while i + 1 < n and rbsp[i] != 0x80:
        ptype, i = ff_coded(i)
        if ptype is None:
            return None
        size, i = ff_coded(i)
        if size is None or i + size > n:
            return None
        if ptype == 6:
            bits = "".join("{:08b}".format(b) for b in rbsp[i:i + size])
            lz = len(bits) - len(bits.lstrip("0"))
            if not bits[lz:] or 2 * lz + 1 > len(bits):
                return None
            return int(bits[lz:2 * lz + 1], 2) - 1
        i += size
    return None


def recovery_points(stream):
    """[(offset, recovery_frame_cnt)] of every recovery point SEI NAL unit of an Annex-B byte string: offset of its start code -
    where a receiver may cut in - and the count of pictures after it until every sample is right"""
    data, spans = _nal_spans(stream)
    out = []
    for sc, nal, end in spans:
        if nal < end and (data[nal] & 0x1F) == 6:
            cnt = _recovery_frame_cnt(_rbsp(data[nal + 1:end]))
            if cnt is not None:
                out.append((sc, cnt))
    return out
