"""Motion-JPEG for the video scripts: the tables and headers of a baseline JPEG encoder and the device encoder's wrapper
(csrc/jpeg.hip), the frame-number stamp, a minimal AVI writer and reader, and the JPEG header parser with the device decoder's
wrapper (csrc/jpeg_decode.hip)."""
import io
import re

import numpy as np
import torch

from .frame_io import device_table

# ---- Motion-JPEG on the device (--device_jpeg 1; csrc/jpeg.hip) -- ITU-T T.81 baseline in a JFIF wrapper, tables of its Annex K ---------
JPEG_RESTART_MCUS = 4          # MCUs (16 x 16 pixels) per restart interval = per wave of the entropy coder: 150 intervals in a 640 x 240 frame
_JPEG_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
_JPEG_LUMA_Q = (16, 11, 10, 16, 24, 40, 51, 61,             # table K.1, rows = vertical frequency
                12, 12, 14, 19, 26, 58, 60, 55,
                14, 13, 16, 24, 40, 57, 69, 56,
                14, 17, 22, 29, 51, 87, 80, 62,
                18, 22, 37, 56, 68, 109, 103, 77,
                24, 35, 55, 64, 81, 104, 113, 92,
                49, 64, 78, 87, 103, 121, 120, 101,
                72, 92, 95, 98, 112, 100, 103, 99)
_JPEG_CHROMA_Q = (17, 18, 24, 47, 99, 99, 99, 99,           # table K.2
                  18, 21, 26, 66, 99, 99, 99, 99,
                  24, 26, 56, 99, 99, 99, 99, 99,
                  47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
# tables K.3 - K.6: (number of codes of length 1..16, symbols in code order); an AC symbol is run << 4 | category
_JPEG_HUFF = (
    ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),                                   # DC luminance
    ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125),                                                    # AC luminance
     (0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
      0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
      0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
      0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
      0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
      0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
      0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
      0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
      0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa)),
    ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),                                   # DC chrominance
    ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119),                                                    # AC chrominance
     (0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
      0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
      0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
      0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
      0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
      0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
      0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
      0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
      0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa)),
)
_JPEG_TABLES, _JPEG_HEADERS = {}, {}


def jpeg_tables(quality):
    """The tables egne_jpeg_encode takes (include/egne_hip.h), as NumPy arrays: (qt uint8 [2,64], the luminance / chrominance divisors
    in zigzag order -- libjpeg's quality scaling of tables K.1 / K.2 --, huff uint32 [544], (code length << 16) | code of the four
    Annex K code tables, dct int32 [8,8], T[u][x] = rint(8192 a(u) cos((2x+1) u pi / 16)) computed in float64).  Cached."""
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError("JPEG quality %d outside 1..100" % quality)
    if quality not in _JPEG_TABLES:
        scale = 5000 // quality if quality < 50 else 200 - 2 * quality
        qt = np.array([[min(max((base[n] * scale + 50) // 100, 1), 255) for n in _JPEG_ZIGZAG] for base in (_JPEG_LUMA_Q, _JPEG_CHROMA_Q)], np.uint8)
        huff = np.zeros(544, np.uint32)
        for (counts, symbols), first in zip(_JPEG_HUFF, (0, 32, 16, 288)):
            code, k = 0, 0
            for length in range(1, 17):                     # T.81 Annex C: codes of one length are consecutive, then a zero bit is appended
                for _ in range(counts[length - 1]):
                    huff[first + symbols[k]] = length << 16 | code
                    code, k = code + 1, k + 1
                code <<= 1
        u, x = np.arange(8, dtype=np.float64)[:, None], np.arange(8, dtype=np.float64)[None, :]
        a = np.where(u == 0, np.sqrt(1.0 / 8.0), np.sqrt(2.0 / 8.0))
        dct = np.rint(8192.0 * a * np.cos((2 * x + 1) * u * np.pi / 16)).astype(np.int32)
        _JPEG_TABLES[quality] = (qt, huff, np.ascontiguousarray(dct))
    return _JPEG_TABLES[quality]


def jpeg_header(W, H, quality, restart_mcus=JPEG_RESTART_MCUS):
    """Everything of a frame's JPEG file in front of the entropy-coded scan: SOI, APP0 (JFIF 1.1), two DQT, SOF0 (8 bit, H x W, Y 2x2,
    Cb 1x1, Cr 1x1), the four DHT, DRI, SOS.  ``restart_mcus`` 1..8: what egne_jpeg_encode's LDS staging is sized for.  Cached."""
    W, H, quality, restart_mcus = int(W), int(H), int(quality), int(restart_mcus)
    if not (1 <= W <= 65535 and 1 <= H <= 65535 and 1 <= restart_mcus <= 8):
        raise ValueError("JPEG frame %dx%d / restart interval %d out of range (1..65535, 1..8 MCUs)" % (W, H, restart_mcus))
    key = (W, H, quality, restart_mcus)
    if key not in _JPEG_HEADERS:
        _JPEG_HEADERS[key] = _build_jpeg_header(*key)
    return _JPEG_HEADERS[key]


def _build_jpeg_header(W, H, quality, restart_mcus):
    qt = jpeg_tables(quality)[0]

    def seg(marker, body):
        return bytes((0xFF, marker)) + (len(body) + 2).to_bytes(2, 'big') + body
    h = b'\xff\xd8' + seg(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    h += seg(0xDB, b'\x00' + qt[0].tobytes()) + seg(0xDB, b'\x01' + qt[1].tobytes())
    h += seg(0xC0, b'\x08' + H.to_bytes(2, 'big') + W.to_bytes(2, 'big') + bytes((3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1)))
    for (counts, symbols), tc_th in zip(_JPEG_HUFF, (0x00, 0x10, 0x01, 0x11)):
        h += seg(0xC4, bytes((tc_th,)) + bytes(counts) + bytes(symbols))
    h += seg(0xDD, restart_mcus.to_bytes(2, 'big'))
    return h + seg(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0)))


def encode_jpeg_device(frames_bgr_u8, quality=90, cap=None):
    """Baseline JPEG files of a stack of uint8 BGR device frames [N,H,W,3] (egne_jpeg_encode): returns device tensors (out uint8
    [N,cap], frame n's file in out[n, :lengths[n]]; lengths int32 [N]; flags int32 [N], 1 where the file did not fit ``cap`` bytes --
    its length is then 0).  ``cap`` defaults to the header plus 1.5 bytes per pixel of the frame padded to multiples of 16.  Queues on
    the current stream, no synchronisation."""
    from egne_amd import _lib
    from egne_amd.engine import require_cuda
    f = frames_bgr_u8
    require_cuda(f, "frames_bgr_u8")
    if f.dtype != torch.uint8 or f.dim() != 4 or f.shape[3] != 3 or min(f.shape) < 1:
        raise ValueError("frames_bgr_u8 must be a uint8 [N,H,W,3] tensor")
    f = f.contiguous()
    N, H, W = int(f.shape[0]), int(f.shape[1]), int(f.shape[2])
    header = jpeg_header(W, H, quality, JPEG_RESTART_MCUS)
    if cap is None:
        cap = len(header) + (-(-H // 16) * 16) * (-(-W // 16) * 16) * 3 // 2
    cap = int(cap)
    if cap < 1:
        raise ValueError("cap must be positive")
    qt, huff, dct = device_table(("jpeg", int(quality)), f.device, lambda: jpeg_tables(quality))
    hd, = device_table(("jpeg_header", W, H, int(quality)), f.device, lambda: (np.frombuffer(header, np.uint8).copy(),))
    L = _lib.lib()
    out = torch.empty((N, cap), dtype=torch.uint8, device=f.device)
    lengths = torch.empty(N, dtype=torch.int32, device=f.device)
    flags = torch.empty(N, dtype=torch.int32, device=f.device)
    ws = torch.empty(int(L.egne_jpeg_workspace_bytes(N, H, W)), dtype=torch.uint8, device=f.device)
    _lib.check(L.egne_jpeg_encode(f.data_ptr(), N, H, W, qt.data_ptr(), huff.data_ptr(), dct.data_ptr(), hd.data_ptr(), len(header),
                                  JPEG_RESTART_MCUS, out.data_ptr(), cap, lengths.data_ptr(), flags.data_ptr(), ws.data_ptr(),
                                  _lib.stream_ptr()), "jpeg_encode")
    return out, lengths, flags


_STAMP_PATCH = (16, 64, 8, 10)         # rows, columns, x0, y0 of the patch that holds the frame number: asserted per number below


def frame_number_mask(j, ph=_STAMP_PATCH[0], pw=_STAMP_PATCH[1], x0=_STAMP_PATCH[2], y0=_STAMP_PATCH[3]):
    """The coverage mask of _put_frame_number's text: str(j) in white on a black 'L' canvas at (10, 12), same default font; returns
    the uint8 [ph,pw] patch at origin (x0, y0), which must hold everything PIL draws (asserted)."""
    from PIL import Image, ImageDraw
    canvas = Image.new('L', (max(x0 + pw, 0) + 128, max(y0 + ph, 0) + 64), 0)
    ImageDraw.Draw(canvas).text((10, 12), str(j), fill=255)
    box = canvas.getbbox()
    if box is not None and not (x0 <= box[0] and y0 <= box[1] and box[2] <= x0 + pw and box[3] <= y0 + ph and
                                box[2] < canvas.size[0] and box[3] < canvas.size[1]):
        raise AssertionError("frame number %r covers %r, outside the %dx%d patch at (%d, %d)" % (j, box, pw, ph, x0, y0))
    full = np.asarray(canvas)
    patch = np.zeros((ph, pw), np.uint8)
    ys, xs = max(y0, 0), max(x0, 0)
    patch[ys - y0:, xs - x0:] = full[ys: y0 + ph, xs: x0 + pw]
    return patch


def stamp_numbers_device(frames, numbers):
    """_put_frame_number(frames[n], numbers[n]) on the device, in place (egne_stamp_mask): ``frames`` uint8 [N,H,W,3] BGR on the GPU.
    The host only draws the numbers' small coverage masks.  Current stream, no synchronisation of the device work."""
    masks = torch.from_numpy(np.stack([frame_number_mask(j) for j in numbers]))
    return _stamp_masks_device(frames, masks.to(frames.device))


def _stamp_masks_device(frames, masks):
    from egne_amd import _lib
    from egne_amd.engine import require_cuda
    require_cuda(frames, "frames")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
        raise ValueError("frames must be a contiguous uint8 [N,H,W,3] tensor")
    if masks.dtype != torch.uint8 or masks.dim() != 3 or masks.shape[0] != frames.shape[0]:
        raise ValueError("one uint8 mask per frame")
    N, H, W = (int(v) for v in frames.shape[:3])
    masks = masks.contiguous()
    _lib.check(_lib.lib().egne_stamp_mask(frames.data_ptr(), N, H, W, masks.data_ptr(), int(masks.shape[1]), int(masks.shape[2]),
                                          _STAMP_PATCH[2], _STAMP_PATCH[3], 0, 0, 255, _lib.stream_ptr()), "stamp_mask")
    return frames


def _put_frame_number(img, j):
    """cv2.putText(frame, str(j), (10, 30), FONT_HERSHEY_PLAIN, 2.0, (0, 0, 255), 2) -- PIL's default font instead of Hershey."""
    from PIL import Image, ImageDraw
    im = Image.fromarray(np.ascontiguousarray(img[..., ::-1]))
    ImageDraw.Draw(im).text((10, 12), str(j), fill=(255, 0, 0))
    img[...] = np.asarray(im)[..., ::-1]


class MJPEGWriter:
    """Minimal AVI (RIFF) writer with Motion-JPEG frames encoded by PIL -- stands in for cv2.VideoWriter (evaluate.py:219-221;
    the reference writes mp4v, for which there is no encoder in this image).  Frames are BGR uint8 arrays as OpenCV's are."""

    def __init__(self, path, fps, size):
        self.path, self.fps, self.size, self.frames = path, max(int(fps), 1), (int(size[0]), int(size[1])), []

    def write(self, frame_bgr):
        from PIL import Image
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(frame_bgr[..., ::-1])).save(buf, format='JPEG', quality=90)
        self.frames.append(buf.getvalue())

    def write_jpeg(self, data):
        """Append a frame that is a complete JPEG file already (encode_jpeg_device)."""
        self.frames.append(bytes(data))

    def release(self):
        import struct
        W, H, n = self.size[0], self.size[1], len(self.frames)
        chunks, idx, off = [], [], 4
        for f in self.frames:
            pad = len(f) & 1
            chunks.append(b'00dc' + struct.pack('<I', len(f)) + f + b'\0' * pad)
            idx.append(b'00dc' + struct.pack('<III', 0x10, off, len(f)))
            off += 8 + len(f) + pad
        movi = b'movi' + b''.join(chunks)
        biggest = max((len(f) for f in self.frames), default=0)
        avih = struct.pack('<IIIIIIIIIIIIII', 1000000 // self.fps, biggest * self.fps, 0, 0x10, n, 0, 1, biggest, W, H, 0, 0, 0, 0)
        strh = b'vids' + b'MJPG' + struct.pack('<IHHIIIIIIIIhhhh', 0, 0, 0, 0, 1, self.fps, 0, n, biggest, 0xffffffff, 0, 0, 0, W, H)
        strf = struct.pack('<IiiHHIIiiII', 40, W, H, 1, 24, 0x47504a4d, W * H * 3, 0, 0, 0, 0)

        def ck(tag, data):
            return tag + struct.pack('<I', len(data)) + data + (b'\0' if len(data) & 1 else b'')

        def lst(tag, data):
            return b'LIST' + struct.pack('<I', len(data) + 4) + tag + data
        hdrl = lst(b'hdrl', ck(b'avih', avih) + lst(b'strl', ck(b'strh', strh) + ck(b'strf', strf)))
        body = b'AVI ' + hdrl + b'LIST' + struct.pack('<I', len(movi)) + movi + ck(b'idx1', b''.join(idx))
        with open(self.path, 'wb') as f:
            f.write(b'RIFF' + struct.pack('<I', len(body)) + body)


def mjpeg_frames(path):
    """Yield grey frames of an MJPEG .avi by scanning for JPEG SOI/EOI markers (no OpenCV)."""
    from PIL import Image
    for chunk in mjpeg_chunks(path):
        try:
            yield np.asarray(Image.open(io.BytesIO(chunk)).convert('L'))
        except Exception:
            continue


def mjpeg_chunks(path):
    """Yield the JPEG files of an MJPEG .avi as byte strings: the SOI/EOI scan, nothing decoded."""
    data = open(path, 'rb').read()
    pos = 0
    while True:
        a = data.find(b'\xff\xd8\xff', pos)
        if a < 0:
            return
        b = data.find(b'\xff\xd9', a)
        if b < 0:
            return
        pos = b + 2
        yield data[a:b + 2]


def _decode_host(data):
    """The host path of a frame: PIL, as mjpeg_frames; None where PIL cannot decode it."""
    from PIL import Image
    try:
        return np.array(Image.open(io.BytesIO(data)).convert('L'))
    except Exception:
        return None


# ---- Motion-JPEG decoding on the device (--device_decode 1; csrc/jpeg_decode.hip) ------------------------------------------------------
JPEG_GREY, JPEG_444, JPEG_422, JPEG_420 = 0, 1, 2, 3          # `sampling` of egne_jpeg_decode
JPEG_DESC_BYTES = 1408                                        # one frame's record of egne_jpeg_decode (include/egne_hip.h)
_JPEG_FOREIGN_MARKER = re.compile(b'\xff[^\x00\xd0-\xd7]')     # in a scan: anything but stuffing and RSTm (a second scan, fill bytes, ...)
_PARSED_HEADER = [None, None]                                 # the last header jpeg_parse walked, and what it found there


def _parse_header(data):
    """The marker segments of a JPEG file up to and including SOS: a dictionary (see jpeg_parse; 'scan_off' = where the scan starts,
    'record' = the frame's descriptor without its scan), or None."""
    n = len(data)
    if n < 4 or data[:2] != b'\xff\xd8':
        return None
    p, qt, huff, restart, sof = 2, {}, {}, 0, None
    while True:
        if p + 4 > n or data[p] != 0xFF:
            return None
        m = data[p + 1]
        L = int.from_bytes(data[p + 2: p + 4], 'big')
        if m in (0x01, 0xD8, 0xD9, 0xFF) or 0xD0 <= m <= 0xD7 or L < 2 or p + 2 + L > n:
            return None
        b = data[p + 4: p + 2 + L]
        if m == 0xDB:
            for k in range(0, len(b), 65):
                if b[k] > 3 or k + 65 > len(b):                # 16-bit divisors (Pq = 1), a table number above 3, a short segment
                    return None
                qt[b[k]] = b[k + 1: k + 65]
        elif m == 0xC4:
            k = 0
            while k < len(b):
                if k + 17 > len(b):
                    return None
                counts = b[k + 1: k + 17]
                nsym, code = sum(counts), 0
                for length in range(16):                       # the codes must fit their lengths (T.81 Annex C)
                    code = (code + counts[length]) << 1
                    if code > 2 << (length + 1):
                        return None
                if b[k] not in (0x00, 0x01, 0x10, 0x11) or nsym > 256 or k + 17 + nsym > len(b):
                    return None
                huff[b[k]] = (bytes(counts), bytes(b[k + 17: k + 17 + nsym]))
                k += 17 + nsym
        elif m == 0xC0:
            if sof is not None or len(b) < 6 or b[0] != 8 or len(b) != 6 + 3 * b[5]:
                return None
            sof = (int.from_bytes(b[1:3], 'big'), int.from_bytes(b[3:5], 'big'),
                   [(b[6 + 3 * i], b[7 + 3 * i] >> 4, b[7 + 3 * i] & 15, b[8 + 3 * i]) for i in range(b[5])])
        elif 0xC1 <= m <= 0xCF:                                # every other frame type: extended, progressive, lossless, arithmetic
            return None
        elif m == 0xDD:
            if len(b) != 2:
                return None
            restart = int.from_bytes(b, 'big')
        elif m == 0xEE and b[:5] == b'Adobe' and len(b) >= 12 and b[11] != 1:
            return None                                        # Adobe transform 0 / 2: the components are RGB or YCCK, not YCbCr
        elif m == 0xDA:
            break
        p += 2 + L
    if sof is None:
        return None
    H, W, comps = sof
    shape = [(h, v) for _, h, v, _ in comps]
    sampling = {((1, 1),): JPEG_GREY, ((1, 1),) * 3: JPEG_444, ((2, 1), (1, 1), (1, 1)): JPEG_422,
                ((2, 2), (1, 1), (1, 1)): JPEG_420}.get(tuple(shape))
    if sampling is None or H < 1 or W < 1:
        return None
    if len(comps) == 3 and [c[0] for c in comps] != [1, 2, 3]:   # libjpeg takes other identifiers ('R', 'G', 'B', ...) for other colour spaces
        return None
    if sampling in (JPEG_422, JPEG_420) and (W + 1) // 2 <= 2:          # libjpeg replicates chroma planes this narrow
        return None
    if len(b) != 4 + 2 * len(comps) or b[0] != len(comps) or tuple(b[-3:]) != (0, 63, 0):
        return None
    if not huff:                                               # AVI Motion-JPEG convention: no DHT = the tables of Annex K
        huff = {ident: (bytes(c), bytes(sy)) for ident, (c, sy) in zip((0x00, 0x10, 0x01, 0x11), _JPEG_HUFF)}
    sel = []
    for i, (ident, _, _, tq) in enumerate(comps):
        td, ta = b[2 + 2 * i] >> 4, b[2 + 2 * i] & 15
        if b[1 + 2 * i] != ident or td > 1 or ta > 1 or td not in huff or 0x10 | ta not in huff or tq not in qt:
            return None
        sel.append((tq, td, ta))
    record = np.zeros(JPEG_DESC_BYTES, np.uint8)
    words = record[:32].view(np.int32)
    words[2] = restart
    for k in range(3):
        words[3 + k] = sum(sl[k] << (8 * c) for c, sl in enumerate(sel))
    for t, body in qt.items():
        record[32 + 64 * t: 96 + 64 * t] = np.frombuffer(body, np.uint8)
    tables = []
    for t, ident in enumerate((0x00, 0x01, 0x10, 0x11)):
        tables.append(huff.get(ident))
        if ident in huff:
            counts, symbols = huff[ident]
            record[288 + 272 * t: 304 + 272 * t] = np.frombuffer(counts, np.uint8)
            record[304 + 272 * t: 304 + 272 * t + len(symbols)] = np.frombuffer(symbols, np.uint8)
    return dict(H=H, W=W, sampling=sampling, components=[(h, v) + sl for (_, h, v, _), sl in zip(comps, sel)],
                qt={t: bytes(body) for t, body in qt.items()}, huff=tables, restart=restart, scan_off=p + 2 + L, record=record)


def jpeg_parse(data):
    """What egne_jpeg_decode needs of one JPEG file, or None for a file the device decoder does not take (anything but SOF0, 8 bit,
    one scan, grey or three components at 4:4:4 / 4:2:2 / 4:2:0, 8-bit quantisation tables; fill bytes or foreign markers inside the
    scan; subsampled chroma planes of one or two columns; three components that are not YCbCr: an Adobe segment with a transform
    other than 1, or identifiers other than 1, 2, 3).  Walks the marker segments only -- byte-level work, nothing per Huffman
    symbol.  Returns a dictionary: H, W, sampling (JPEG_GREY / JPEG_444 / JPEG_422 / JPEG_420), components [(h, v, tq, td, ta)],
    qt {table: 64 bytes in file (zigzag) order}, huff [DC 0, DC 1, AC 0, AC 1] as (16 counts, symbols) or None (a file without DHT
    gets the tables of Annex K), restart (MCUs, 0 = none), scan_off, scan_len (the entropy-coded scan: up to EOI), record."""
    hdr, info = _PARSED_HEADER
    if hdr is None or not data.startswith(hdr):                # (a video's frames mostly share their header byte for byte)
        info = _parse_header(data)
        if info is None:
            return None
        _PARSED_HEADER[:] = [bytes(data[:info['scan_off']]), info]
    off = info['scan_off']
    end = data.find(b'\xff\xd9', off)
    if end < 0 or _JPEG_FOREIGN_MARKER.search(data, off, end) or data[end - 1: end] == b'\xff':
        return None
    return dict(info, scan_len=end - off)


def decode_jpeg_device(datas, device=None, sub_bits=1024, mode=1, out=None, parsed=None):
    """Grey frames of a list of baseline JPEG files (byte strings) decoded on the device (egne_jpeg_decode): returns (grey uint8
    [N,H,W] on the device -- byte for byte np.asarray(Image.open(...).convert('L')) of every file --, flags int32 [N], non-zero where
    the scan turned out invalid: that frame's row is then unspecified).  All files share H, W and sampling (ValueError otherwise, and
    for a file jpeg_parse refuses).  ``mode`` 1: self-synchronising subsequences of ``sub_bits`` bits; 0: one lane per restart
    interval.  ``out``: the uint8 [N,H,W] device tensor to decode into; ``parsed``: the files' jpeg_parse results, if the caller has
    them.  One upload of the concatenated scans and one of the descriptor table; queues on the current stream, no synchronisation."""
    from egne_amd import _lib
    datas = list(datas)
    infos = [jpeg_parse(d) for d in datas] if parsed is None else list(parsed)
    if not datas or len(infos) != len(datas):
        raise ValueError("decode_jpeg_device needs at least one JPEG file (and one jpeg_parse result per file)")
    for n, info in enumerate(infos):
        if info is None:
            raise ValueError("file %d is not a JPEG stream the device decoder takes (jpeg_parse)" % n)
    H, W, sampling = infos[0]['H'], infos[0]['W'], infos[0]['sampling']
    for n, info in enumerate(infos):
        if (info['H'], info['W'], info['sampling']) != (H, W, sampling):
            raise ValueError("file %d is %dx%d with sampling %d, file 0 %dx%d with sampling %d: one call, one geometry"
                             % (n, info['H'], info['W'], info['sampling'], H, W, sampling))
    N = len(datas)
    desc = np.stack([info['record'] for info in infos])
    words = desc[:, :32].view(np.int32)
    parts, at = [], 0
    for n, (d, info) in enumerate(zip(datas, infos)):
        scan = d[info['scan_off']: info['scan_off'] + info['scan_len']]
        words[n, 0], words[n, 1] = at, len(scan)
        parts += [scan, b'\0' * (-len(scan) % 4)]
        at += len(scan) + (-len(scan) % 4)
    nbytes = max(at, 4)
    device = torch.device('cuda' if device is None else device)
    streams = torch.from_numpy(np.frombuffer(b''.join(parts).ljust(nbytes, b'\0'), np.uint8).copy()).to(device)
    desc = torch.from_numpy(desc).to(device)
    if out is None:
        out = torch.empty((N, H, W), dtype=torch.uint8, device=device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (N, H, W) or not out.is_contiguous() or out.device.type != 'cuda':
        raise ValueError("out must be a contiguous uint8 [%d,%d,%d] tensor on the device" % (N, H, W))
    L = _lib.lib()
    flags = torch.empty(N, dtype=torch.int32, device=device)
    ws = torch.empty(int(L.egne_jpeg_decode_workspace_bytes(N, H, W, sampling, nbytes, int(sub_bits), 1)), dtype=torch.uint8, device=device)
    _lib.check(L.egne_jpeg_decode(streams.data_ptr(), nbytes, desc.data_ptr(), N, H, W, sampling, int(sub_bits), int(mode), out.data_ptr(),
                                  None, flags.data_ptr(), None, ws.data_ptr(), _lib.stream_ptr()), "jpeg_decode")
    return out, flags
