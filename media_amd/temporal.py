"""Temporal layers on the receiving side: what a forwarding server needs to thin a two-layer stream (include/mi355x_h264.h,
"temporal layers").  A layer-1 picture is a P picture nobody refers to: its slice NAL units carry nal_ref_idc 0, and a stream
without them still decodes - to the layer-0 pictures.  Plain Python on Annex-B bytes; no device, no library."""

_SLICE_TYPES = (1, 5)     # nal_unit_type of a coded slice: non-IDR, IDR


def _nal_spans(data):
    """(start of the start code, start of the NAL unit, end) of every NAL unit of an Annex-B byte string; three- and four-byte
    start codes; trailing zero bytes in front of a start code belong to that start code"""
    data = bytes(data)
    starts, i = [], data.find(b"\x00\x00\x01")
    while i >= 0:
        starts.append(i)
        i = data.find(b"\x00\x00\x01", i + 3)
    spans = []
    for k, s in enumerate(starts):
        end = starts[k + 1] if k + 1 < len(starts) else len(data)
        while k + 1 < len(starts) and end > s + 3 and data[end - 1] == 0:
            end -= 1
        sc = s
        while sc > (spans[-1][2] if spans else 0) and data[sc - 1] == 0:
            sc -= 1
        spans.append((sc, s + 3, end))
    return data, spans


def _is_layer1(hdr):
    return (hdr & 0x1F) in _SLICE_TYPES and (hdr >> 5) & 3 == 0


def base_layer(annexb_bytes):
    """the stream without its layer-1 pictures: the slice NAL units of nal_ref_idc 0 dropped, everything else byte for byte"""
    data, spans = _nal_spans(annexb_bytes)
    return b"".join(data[sc:end] for sc, nal, end in spans if nal < end and not _is_layer1(data[nal]))


def layers(annexb_bytes):
    """(base, enhancement): the two layers' NAL units, each with its start code, in stream order.  Parameter sets and everything
    that is no slice go with the base layer"""
    data, spans = _nal_spans(annexb_bytes)
    base, enh = [], []
    for sc, nal, end in spans:
        if nal < end:
            (enh if _is_layer1(data[nal]) else base).append(data[sc:end])
    return b"".join(base), b"".join(enh)
