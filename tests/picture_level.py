"""Random streams with picture-level variety (oracle/h264_enc.c h264o_enc_random_picture, features 16384 / 32768 / 65536):
non-reference pictures, I and P slices in any non-IDR picture, several parameter sets and left / top cropping.  The case list
and the helpers the CPU tests (tests/test_dec_parser.py) and the GPU tests (tests/test_gpu_decoder.py,
tests/test_gpu_decoder_plugin.py) share."""
import annexb
from oracle_lib import OracleEncoder

N, S, P = OracleEncoder.RAND_NONREF, OracleEncoder.RAND_SLICE_TYPES, OracleEncoder.RAND_PARAMETER_SETS

# width, height, profile_idc, slices, refs, features: each bit alone, each pair, all three, all three with 63 | 128 | 256 | 1024;
# one, two and three reference pictures; one slice, bands of rows, slices cut anywhere (64, which needs 32); every profile;
# 16x16 is a single macroblock (one slice, so one slice type per picture: ring arithmetic only).  Bit 256 (POC type 0) is what
# allows runs of two and three non-reference pictures.
PICTURE_LEVEL_CASES = [
    (96, 80, 66, 0, 1, N),
    (96, 80, 77, 2, 2, S),
    (112, 64, 100, 3, 3, P),
    (112, 64, 66, 3, 3, N | S | 128),
    (96, 80, 100, 2, 2, N | P | 256 | 1),
    (48, 32, 77, 0, 3, S | P | 32 | 64),
    (96, 80, 100, 3, 2, N | S | P),
    (112, 64, 100, 2, 3, N | S | P | 63 | 128 | 256 | 1024),
    (16, 16, 66, 0, 2, N | S | P | 256),
    (48, 32, 66, 0, 1, N | S | P | 32 | 64 | 256 | 1),
    (96, 80, 77, 3, 3, N | S | P | 256 | 128 | 31),
]
PICTURES, GOP = 16, 5


def seed(case, i):
    w, h, prof, slices, refs, features = case
    return 15485863 * i + 7 * w + 3 * prof + 11 * slices + refs + features


def encoder(case, gop=GOP):
    w, h, prof, slices, refs, features = case
    return OracleEncoder(w, h, qp=30, gop=gop, profile_idc=prof, slices=slices, refs=refs)


def pictures(case, n=PICTURES, gop=GOP):
    """the case's stream: a list of (access unit, is_idr, is_ref), and the generator's hit counters over it"""
    enc = encoder(case, gop)
    out = []
    for i in range(n):
        au, idr, _ = enc.random_picture(seed(case, i), features=case[5])
        out.append((au, idr, bool(enc.random_last()["is_ref"])))
    hits = enc.hits()
    enc.close()
    return out, hits


def thinned(aus):
    """The stream without its non-reference pictures: every slice NAL unit of nal_ref_idc 0 is removed.  A parameter set that
    travelled in front of such a picture stays in the stream (it moves to the front of the next access unit that is kept):
    later pictures may name it, and dropping a picture never entitles anyone to drop a parameter set.  Returns the access
    units that remain, and for each the index of the picture it was."""
    out, index, pending = [], [], b""
    for i, au in enumerate(aus):
        kept, vcl = pending, False
        for ref, typ, payload in annexb.split_nal_units(au):
            if typ in (1, 5) and ref == 0:
                continue
            vcl |= typ in (1, 5)
            kept += b"\x00\x00\x00\x01" + bytes([(ref << 5) | typ]) + payload
        if vcl:
            out.append(kept)
            index.append(i)
            pending = b""
        else:
            pending = kept
    return out, index
