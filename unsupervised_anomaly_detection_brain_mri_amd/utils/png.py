"""utils/png.py -- a minimal PNG codec on zlib for the evaluation sample images (the reference's imageio.imwrite, utils/Evaluation.py:302-321):
no imageio, cv2 or PIL dependency.  write_png writes 8-bit greyscale, RGB and RGBA (colour types 0, 2, 6), filter 0 on every row, one IDAT
chunk, correct CRCs; read_png reads what write_png writes."""
import struct
import zlib

import numpy as np

SIGNATURE = b'\x89PNG\r\n\x1a\n'
_COLOUR_TYPE = {1: 0, 3: 2, 4: 6}          # channels -> PNG colour type
_CHANNELS = {0: 1, 2: 3, 6: 4}


def _chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode_png(a, level=6):
    """uint8 [H,W], [H,W,3] or [H,W,4] -> the bytes of a PNG file."""
    a = np.asarray(a)
    if a.dtype != np.uint8:
        raise TypeError(f'write_png takes uint8 arrays, got {a.dtype}')
    if a.ndim == 2:
        a = a[..., None]
    if a.ndim != 3 or a.shape[2] not in _COLOUR_TYPE or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f'write_png takes [H,W], [H,W,3] or [H,W,4] with H, W >= 1, got {a.shape}')
    h, w, c = a.shape
    rows = np.zeros((h, 1 + w * c), np.uint8)              # every row: filter type 0, then the pixels
    rows[:, 1:] = a.reshape(h, w * c)
    ihdr = struct.pack('>IIBBBBB', w, h, 8, _COLOUR_TYPE[c], 0, 0, 0)
    return SIGNATURE + _chunk(b'IHDR', ihdr) + _chunk(b'IDAT', zlib.compress(rows.tobytes(), level)) + _chunk(b'IEND', b'')


def write_png(path, a, level=6):
    data = encode_png(a, level)
    with open(path, 'wb') as f:
        f.write(data)


def decode_png(data):
    if data[:8] != SIGNATURE:
        raise ValueError('not a PNG file')
    pos, ihdr, idat = 8, None, b''
    while pos < len(data):
        n, kind = struct.unpack('>I4s', data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        crc, = struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])
        if len(body) != n or zlib.crc32(kind + body) & 0xFFFFFFFF != crc:
            raise ValueError(f'PNG chunk {kind!r}: bad length or CRC')
        pos += 12 + n
        if kind == b'IHDR':
            ihdr = struct.unpack('>IIBBBBB', body)
        elif kind == b'IDAT':
            idat += body
        elif kind == b'IEND':
            break
    if ihdr is None:
        raise ValueError('PNG file without IHDR')
    w, h, depth, ctype, comp, flt, interlace = ihdr
    if depth != 8 or ctype not in _CHANNELS or comp or flt or interlace:
        raise ValueError('read_png reads 8-bit colour types 0, 2, 6 without interlace only')
    c = _CHANNELS[ctype]
    rows = np.frombuffer(zlib.decompress(idat), np.uint8)
    if rows.size != h * (1 + w * c):
        raise ValueError('PNG image data of the wrong size')
    rows = rows.reshape(h, 1 + w * c)
    if rows[:, 0].any():
        raise ValueError('read_png reads filter type 0 only')
    a = rows[:, 1:].reshape(h, w, c).copy()
    return a[..., 0] if c == 1 else a


def read_png(path):
    """-> uint8 [H,W], [H,W,3] or [H,W,4] of a file written by write_png."""
    with open(path, 'rb') as f:
        return decode_png(f.read())
