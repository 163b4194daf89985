"""zip-ada_amd -- MI355X-native Deflate encoder behind the Zip-Ada `Zip.Compress` interface.

Host-side mirror of the reference's interface for the hot path (the reference is Ada; no Ada
toolchain exists in the build image, so the host side above the C ABI is written here and in
`csrc/`; see INTEGRATION.md for the Ada shim a maintainer would add):

    Compression_Method        zip_lib/zip-compress.ads:59-122   -> `Method`
    Zip.Compress.Deflate      zip_lib/zip-compress-deflate.ads:36-46 -> `Encoder.deflate`
    Zip.Compress.Compress_Data zip_lib/zip-compress.ads:169-180 -> `Encoder.compress_data`
    Zip.Create (Create_Archive / Add_Stream / Finish) zip_lib/zip-create.ads:75-211 -> `ZipCreate`
    Zip.CRC_Crypto (Init_Keys / Encode) zip_lib/zip-crc_crypto.adb:90-128 -> `Encoder.crypt_*`, `password=` of `compress_data` / `ZipCreate`

All compute runs in libzada_hip.so (hand-written HIP for gfx950).  There is no CPU fallback:
loading fails loudly when the library or a GPU is missing.
"""
import ctypes
import os
import struct

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ZADA_LIB", os.path.join(_HERE, "libzada_hip.so"))   # ZADA_LIB: A/B builds of the same library


class Method:
    """Compression_Method'Pos, zip-compress.ads:59-122.  Every method has an encoder (Encoder.shrink / reduce / deflate / bzip2 / lzma and their batch
    calls, compress_data, ZipCreate); the Preselection methods pick one of the others per entry (preselect) and never Shrink or Reduce.  Shrink_1
    and Reduce_1 .. _4 in the device tools are opt-in: Encoder.zip_device_ex / ZipCreate.write_device_ex (..., legacy=True) write them, ReZip (encoder,
    legacy=True) tries shrink and reduce_4 and reads such sources; without the keyword they are refused by name.  zip_device (Store and Deflate only)
    refuses them always.  Reading such entries -- and Implode entries, which have no encoder here -- is opt-in as well: Encoder.unlegacy*,
    UnZip / CompZip / FindZip (encoder, legacy=True); without the keyword they stay UnsupportedMethod."""
    Store = 0
    Shrink_1 = 1
    Reduce_1, Reduce_2, Reduce_3, Reduce_4 = 2, 3, 4, 5
    Deflate_Fixed = 6
    Deflate_0 = 7
    Deflate_1 = 8
    Deflate_2 = 9
    Deflate_3 = 10
    Deflate_R = 11
    BZip2_1, BZip2_2, BZip2_3 = 12, 13, 14
    LZMA_0, LZMA_1, LZMA_2, LZMA_3 = 15, 16, 17, 18
    LZMA_2_for_Zip_in_Zip, LZMA_3_for_Zip_in_Zip = 19, 20
    LZMA_2_for_Source, LZMA_3_for_Source = 21, 22
    LZMA_for_JPEG, LZMA_for_ARW, LZMA_for_ORF, LZMA_for_MP3, LZMA_for_MP4 = 23, 24, 25, 26, 27
    LZMA_for_PGM, LZMA_for_PPM, LZMA_for_PNG, LZMA_for_GIF, LZMA_for_WAV, LZMA_for_AU = 28, 29, 30, 31, 32, 33
    Preselection_1, Preselection_2 = 34, 35


class ContentType:
    """Data_Content_Type'Pos, zip-compress.ads:151-160: the content hint of the Preselection methods."""
    neutral = 0
    source_code = 1
    text_formatted_text_or_dna = 2
    text_data = 3
    JPEG = 4
    ARW_RW2 = 5
    ORF_CR2 = 6
    Zip_in_Zip = 7
    GIF, PNG, PGM, PPM = 8, 9, 10, 11
    WAV = 12
    AU = 13
    MP3, MP4 = 14, 15


def _zip_type(method):
    """The Zip format code of a single method (zip.ads:496-503): Shrink 1, Reduce_1 .. _4 2 .. 5, BZip2 12, LZMA 14, Deflate 8, Store 0."""
    if Method.Shrink_1 <= method <= Method.Reduce_4:
        return int(method)
    return 0 if method == Method.Store else 12 if Method.BZip2_1 <= method <= Method.BZip2_3 else 14 if Method.LZMA_0 <= method <= Method.LZMA_for_AU else 8


def guess_type_from_name(name):
    """Zip.Compress.Guess_Type_from_Name (zip-compress.adb:330-424): the ContentType of an entry name (zada_guess_type_from_name)."""
    return int(load_library().zada_guess_type_from_name(name.encode("utf-8") if isinstance(name, str) else bytes(name)))


def preselect(method, content_hint=ContentType.neutral, input_size=None):
    """The single method Compress_Data uses for `method` (zip-compress.adb:243-327; zada_preselect): Preselection_1 / _2 by the content
    hint and, when known, the input size; a single method is returned as it is."""
    m = load_library().zada_preselect(int(method), int(content_hint), 0 if input_size is None else 1, 0 if input_size is None else int(input_size))
    if m < 0:
        raise ZadaError("zada_preselect: method %d or content hint %d out of range" % (method, content_hint))
    return int(m)


E_REFERENCE = -6     # zada.h ZADA_E_REFERENCE: LZMA_3, the reference's own matcher reports a match that is none on this entry
E_DATA = -7          # zada.h ZADA_E_DATA: zada_inflate* / zada_bunzip2* / zada_unlzma*, the compressed data is not a valid stream
E_PASSWORD = -8      # zada.h ZADA_E_PASSWORD: zada_unzip_device, the decoded encryption header does not end in the entry's check byte


class ZadaError(RuntimeError):
    pass


class ReferenceDefect(ZadaError):
    """ZADA_E_REFERENCE: on this LZMA_3 entry the reference's BT4 matcher reports a match that is none (include/zada.h); the reference's own
    stream would not decode to the input, nothing was written."""


class DataError(ZadaError):
    """ZADA_E_DATA: the compressed data is not a valid Deflate / Deflate64 stream, or writes more than the size promised (Zip.Archive_corrupted)."""


class WrongPassword(ZadaError):
    """UnZip.Wrong_password (unzip.ads:276-283): the decoded encryption header does not end in the entry's check byte."""


class SizeError(ZadaError):
    """UnZip.Uncompressed_Size_Error: the entry decodes to another size than the directory says."""


class CRCError(ZadaError):
    """UnZip.CRC_Error: the CRC-32 of the decoded bytes is not the directory's."""


class UnsupportedMethod(ZadaError):
    """UnZip.Unsupported_method: the reader decodes Store (0), Deflate (8) and Deflate64 (9); BZip2, LZMA and the older formats are out of its scope."""


class CompressionInefficient(Exception):
    """zip-compress.ads:237 -- compressed size >= uncompressed size."""


class UserAbort(Exception):
    """zip-compress.ads:149."""


RZ_APPROACHES = ("original", "presel_2", "presel_1", "shrink", "reduce_4", "deflate_3", "deflate_r", "bzip2_3", "bzip2_2", "bzip2_1", "lzma_3", "lzma_2")
RZ_DEFAULT = 0x0FE7                                  # zada.h ZADA_RZ_DEFAULT: every approach but shrink and reduce_4
RZ_LEGACY = 0x0018                                   # shrink and reduce_4: taken with the knob "zip_legacy" (ReZip (encoder, legacy=True))
RZ_ALL_FORMATS, RZ_DEFLATE_OR_STORE, RZ_FAST_DECOMPRESSION = 0x1F, 0x03, 0x17       # bits: Store, Deflate, Deflate64, BZip2, LZMA (rezip_lib.ads:46-54)
RZ_NOT_TRIED = 0xFFFFFFFFFFFFFFFF

_lib = None


def load_library():
    """Loads libzada_hip.so.  Raises ZadaError if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ZadaError("libzada_hip.so is missing: run __graft_entry__.build() "
                        "(make -C zip-ada_amd/csrc). There is no CPU fallback.")
    # One HIP runtime per process: PyTorch bundles its own libamdhip64 / libhsa-runtime64.  If this library pulled in
    # /opt/rocm's copy first, a later `import torch` would bring up a SECOND runtime in the same process, which on some
    # nodes cannot open the GPU any more ("No HIP GPUs are available").  Loaded after torch, libzada_hip.so binds to the
    # runtime torch has loaded (same soname).  PyTorch is only plumbing here (device buffers, torch.distributed).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, u64, u32p, u64p, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64), ctypes.c_int
    L.zada_create.restype = vp
    L.zada_create.argtypes = [i32]
    L.zada_destroy.argtypes = [vp]
    L.zada_last_error.restype = ctypes.c_char_p
    L.zada_last_error.argtypes = [vp]
    L.zada_version.restype = ctypes.c_char_p
    L.zada_deflate.argtypes = [vp, i32, vp, u64, vp, u64, u64p, u32p, vp, vp]
    L.zada_deflate_device.argtypes = [vp, i32, vp, u64, vp, u64, u64p, u32p]
    L.zada_deflate_batch.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.zada_compress_data.argtypes = [vp, i32, vp, u64, vp, u64, u64p, u32p, ctypes.POINTER(ctypes.c_uint16)]
    L.zada_lz77_tokens.argtypes = [vp, i32, vp, u64, vp, u64, u64p]
    L.zada_last_blocks.argtypes = [vp, vp, u64, u64p]
    L.zada_last_timing.argtypes = [vp, vp, vp, i32]
    L.zada_last_trace.argtypes = [vp, vp, u64, u64p]
    L.zada_silesia_mix.argtypes = [u64, ctypes.c_uint, u64, u64, vp]
    L.zada_silesia_mix_v2.argtypes = [u64, ctypes.c_uint, u64, u64, vp]
    L.zada_set_knob.argtypes = [vp, ctypes.c_char_p, i32]
    L.zada_range_open.argtypes = [vp, i32, vp, u64, u64, u64, u64, u64]
    L.zada_range_lz.argtypes = [vp, vp, vp]
    L.zada_range_edges.argtypes = [vp, vp, vp, u32p, vp, vp, u32p]
    L.zada_range_place.argtypes = [vp, u64, u64, vp, vp, ctypes.c_uint32, vp, vp, ctypes.c_uint32]
    L.zada_range_analyze.argtypes = [vp]
    L.zada_range_choose.argtypes = [vp, vp, vp, u64p, u64p]
    L.zada_range_emit.argtypes = [vp, vp, u64, u64p]
    L.zada_bzip2.argtypes = [vp, i32, vp, u64, vp, u64, u64p, u32p, vp, vp]
    L.zada_bzip2_device.argtypes = [vp, i32, vp, u64, vp, u64, u64p, u32p]
    L.zada_bz2_range_open.argtypes = [vp, i32, vp, u64, u64, u64, u64, u64, u64p, u64p]
    L.zada_bz2_range_encode.argtypes = [vp]
    L.zada_bz2_range_table.restype = ctypes.c_uint64
    L.zada_bz2_range_table.argtypes = [vp, vp, u64]
    L.zada_bz2_select.restype = None
    L.zada_bz2_select.argtypes = [u64, vp, u64, ctypes.c_uint32, vp, u64p, u32p]
    L.zada_bz2_range_assemble.argtypes = [vp, vp, u64, u64, i32, ctypes.c_uint32, vp, u64, u64p]
    L.zada_crc32_device.argtypes = [vp, vp, u64, u32p]
    L.zada_bzip2_batch.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.zada_lzma.argtypes = [vp, i32, vp, u64, vp, u64, u64p, u32p, vp, vp]
    L.zada_lzma_device.argtypes = [vp, i32, vp, u64, vp, u64, u64p, u32p]
    L.zada_lzma_export_state.argtypes = [vp, vp, u64, u64p, vp, u64, u64p, u64p]
    L.zada_lzma_import_state.argtypes = [vp, vp, u64]
    L.zada_lzma_batch.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.zada_shrink.argtypes = [vp, vp, u64, vp, u64, u64p, u32p]
    L.zada_shrink_device.argtypes = [vp, vp, u64, vp, u64, u64p, u32p]
    L.zada_shrink_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.zada_reduce.argtypes = [vp, i32, vp, u64, vp, u64, u64p, u32p]
    L.zada_reduce_device.argtypes = [vp, i32, vp, u64, vp, u64, u64p, u32p]
    L.zada_reduce_batch.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.zada_reduce_last_record.restype = ctypes.c_uint64
    L.zada_reduce_last_record.argtypes = [vp, i32, ctypes.c_uint32, vp, u64]
    L.zada_lzma_match_sets.argtypes = [vp, vp, u64, vp, vp, vp, i32]
    if hasattr(L, "zada_preselect"):                 # (an older library under ZADA_LIB, for an A/B of what both have, lacks these)
        L.zada_lzma_lit_table_bytes.restype = ctypes.c_uint64
        L.zada_lzma_lit_table_bytes.argtypes = [i32]
        L.zada_guess_type_from_name.argtypes = [ctypes.c_char_p]
        L.zada_preselect.argtypes = [i32, i32, i32, u64]
        L.zada_compress_data_hint.argtypes = [vp, i32, i32, vp, u64, vp, u64, u64p, u32p, vp, vp]
    if hasattr(L, "zada_crypt_encode"):              # (likewise: ZipCrypto)
        L.zada_crypt_init_keys.restype = None
        L.zada_crypt_init_keys.argtypes = [ctypes.c_char_p, u64, u32p]
        L.zada_crypt_header.restype = None
        L.zada_crypt_header.argtypes = [u32p, ctypes.c_char_p, ctypes.c_uint32, vp]
        L.zada_crypt_encode.argtypes = [vp, u32p, vp, u64]
        L.zada_crypt_encode_device.argtypes = [vp, u32p, vp, u64]
        L.zada_crypt_encode_batch.argtypes = [vp, i32, vp, vp, vp]
        L.zada_compress_data_pw.argtypes = [vp, i32, i32, ctypes.c_char_p, u64, ctypes.c_char_p, vp, u64, vp, u64, u64p, u32p, ctypes.POINTER(ctypes.c_uint16), vp]
    if hasattr(L, "zada_inflate"):                   # (likewise: the reader)
        L.zada_inflate.argtypes = [vp, i32, vp, u64, vp, u64, u64p, u64p, u32p]
        L.zada_inflate_device.argtypes = [vp, i32, vp, u64, vp, u64, u64p, u64p, u32p]
        L.zada_inflate_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.zada_crypt_decode_batch.argtypes = [vp, i32, vp, vp, vp]
        L.zada_inflate_par.argtypes = [vp, i32, vp, u64, vp, u64, u64p, u64p, u32p]
        L.zada_inflate_par_device.argtypes = [vp, i32, vp, u64, vp, u64, u64p, u64p, u32p]
        L.zada_inflate_par_last.argtypes = [vp, vp]
    if hasattr(L, "zada_bunzip2"):                   # (likewise: the BZip2 reader)
        L.zada_bunzip2.argtypes = [vp, vp, u64, vp, u64, u64p, u64p, u32p]
        L.zada_bunzip2_device.argtypes = [vp, vp, u64, vp, u64, u64p, u64p, u32p]
        L.zada_bunzip2_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.zada_bunzip2_last_records.restype = u64
        L.zada_bunzip2_last_records.argtypes = [vp, i32, vp, u64]
    if hasattr(L, "zada_unlzma"):                    # (likewise: the LZMA reader)
        L.zada_unlzma.argtypes = [vp, vp, u64, vp, u64, i32, u64p, u64p, u32p]
        L.zada_unlzma_device.argtypes = [vp, vp, u64, vp, u64, i32, u64p, u64p, u32p]
        L.zada_unlzma_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.zada_unlzma_last_records.restype = u64
        L.zada_unlzma_last_records.argtypes = [vp, vp, u64]
    if hasattr(L, "zada_unlegacy"):                  # (likewise: the Shrink / Reduce / Implode reader)
        L.zada_unlegacy.argtypes = [vp, i32, i32, vp, u64, vp, u64, u64p, u64p, u32p]
        L.zada_unlegacy_device.argtypes = [vp, i32, i32, vp, u64, vp, u64, u64p, u64p, u32p]
        L.zada_unlegacy_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.zada_unlegacy_last_records.restype = u64
        L.zada_unlegacy_last_records.argtypes = [vp, vp, u64]
    if hasattr(L, "zada_unzip_device"):              # (likewise: the archive reader on device memory)
        L.zada_unzip_device.argtypes = [vp, vp, u64, vp, u64, i32, vp, u32p, vp]
    if hasattr(L, "zada_zip_device"):                # (likewise: the archive writer on device memory)
        L.zada_zip_bound.restype = u64
        L.zada_zip_bound.argtypes = [i32, vp, u64]
        L.zada_zip_device.argtypes = [vp, i32, i32, vp, vp, u64, u64, u64p, vp]
    if hasattr(L, "zada_zip_device_ex"):             # (likewise: every method, and passwords)
        L.zada_zip_bound_ex.restype = u64
        L.zada_zip_bound_ex.argtypes = [i32, vp, u64, i32]
        L.zada_zip_device_ex.argtypes = [vp, i32, i32, vp, vp, u64, u64, vp, u64p, vp]
    if hasattr(L, "zada_rezip_device"):              # (likewise: ReZip on device memory)
        L.zada_rezip_bound.restype = u64
        L.zada_rezip_bound.argtypes = [i32, vp, u64]
        L.zada_rezip_device.argtypes = [vp, vp, u64, i32, vp, ctypes.c_uint32, ctypes.c_uint32, vp, u64, u64, vp, ctypes.c_uint32, u64p, vp, vp]
    if hasattr(L, "zada_compare_device"):            # (likewise: Comp_Zip on device memory)
        L.zada_compare_device.argtypes = [vp, vp, vp, u64, u64p]
        L.zada_compzip_device.argtypes = [vp, vp, u64, vp, u64, i32, vp, vp, u32p, vp]
    if hasattr(L, "zada_find_device"):               # (likewise: Find_Zip on device memory)
        L.zada_find_device.argtypes = [vp, vp, u64, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, u64p, u64p]
        L.zada_findzip_device.argtypes = [vp, vp, u64, i32, vp, u32p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, vp]
    if hasattr(L, "zada_trained_stub"):              # (likewise: Trained_Compression)
        L.zada_trained_stub.argtypes = [vp, vp, u64, vp, u64, u64p]
        L.zada_trained_open_encoder.argtypes = [vp, vp, u64, i32, u64, ctypes.POINTER(vp)]
        L.zada_trained_open_decoder.argtypes = [vp, vp, u64, u64, u64, ctypes.POINTER(vp)]
        L.zada_trained_encode_device.argtypes = [vp, vp, i32, vp, vp, vp]
        L.zada_trained_decode_device.argtypes = [vp, vp, i32, vp, vp, vp]
        L.zada_trained_info.argtypes = [vp, vp]
        L.zada_trained_close.restype = None
        L.zada_trained_close.argtypes = [vp]
    L.zada_bz2_last_blocks.restype = ctypes.c_uint64
    L.zada_bz2_last_blocks.argtypes = [vp, vp, u64]
    L.zada_crc32_combine.restype = ctypes.c_uint32
    L.zada_crc32_combine.argtypes = [ctypes.c_uint32, ctypes.c_uint32, u64]
    _lib = L
    return L


FEEDBACK_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_int, ctypes.c_void_p)
CARRY_BYTES = 352          # ZADA_CARRY_BYTES
RANGE_ALIGN = 65536        # range boundaries
RANGE_PRE = 32768          # bytes resident before a range that does not start the stream
RANGE_POST = 1 << 20       # ... and behind one that does not end it (or the rest of the stream, if shorter)
EDGE_HEAD, EDGE_TAIL = 65536, 2048


class _ParseState(ctypes.Structure):
    _fields_ = [("pos", ctypes.c_uint64), ("kind", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


class _RangeInfo(ctypes.Structure):
    _fields_ = [("atoms", ctypes.c_uint64), ("exit", _ParseState), ("warm", _ParseState), ("crc_raw", ctypes.c_uint32), ("entry_known", ctypes.c_uint32)]


def _password(password):
    """A password as the bytes Init_Keys sees: Character'Pos of every character, i.e. Latin-1 (zip-crc_crypto.adb:110-116)."""
    pw = password.encode("latin-1") if isinstance(password, str) else bytes(password)
    if not pw:
        raise ZadaError("empty password (Password = \"\" means no encryption, zip-create.adb:221)")
    return pw


FZ_IGNORE_CASE = 1         # ZADA_FZ_IGNORE_CASE
FZ_MAX = 1024              # find_zip.adb's max: the longest search string


def _search_text(text, check=True):
    """A search string as the bytes Find_Zip sees: Character'Pos of every character, i.e. Latin-1, as passwords are.  check: a length outside
    1 .. 1024 is a ValueError (Prepare_Search_String raises Constraint_Error there)."""
    t = text.encode("latin-1") if isinstance(text, str) else bytes(text)
    if check and not 1 <= len(t) <= FZ_MAX:
        raise ValueError("a search string of %d bytes: find_zip takes 1 .. %d" % (len(t), FZ_MAX))
    return t


def _addr(buf):
    """Address of a bytes / bytearray / numpy array / ctypes buffer without copying."""
    if isinstance(buf, bytes):
        return ctypes.cast(ctypes.c_char_p(buf), ctypes.c_void_p).value
    if hasattr(buf, "ctypes"):
        return buf.ctypes.data
    return ctypes.addressof((ctypes.c_char * len(buf)).from_buffer(buf))


class Encoder:
    """One context = one GPU + stream + workspace (single owner, like one Ada task)."""

    def __init__(self, device=0):
        self.lib = load_library()
        self.device = device
        self.ctx = self.lib.zada_create(device)
        if not self.ctx:
            raise ZadaError("zada_create(%d) failed: no usable gfx950 device (no CPU fallback)" % device)

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.zada_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_knob(self, name, value):
        """Tuning / test knobs ("budget", "max_demand_rounds", "inner_budget", "shard_kib", "span_mib", "batch_mib", "bunzip_batch_mib", "inflate_par_chunk_kib", "inflate_par_repair_pct", "inflate_par_min_kib", "inflate_par_deflate64"); none changes a byte of output.
        "inflate_par_batch" = 1: the entries "inflate_par_min_kib" selects in a group of unzip_device go through the same launches instead of one after the other (UnZip (..., parallel_batch=True)
        sets it around its call); "inflate_par_batch_mib" (default 8 192, 1 .. 1 048 576): MiB of symbol workspace one pass of that may promise.
        "inflate_par_deflate64" = 1: inflate_par* and unzip_device's parallel path take Deflate64 (format 9) streams too (UnZip (..., parallel_deflate64=True) sets it around its calls).
        "unzip_legacy" = 1: unzip_device, compzip_device and findzip_device know methods 1 .. 6 (UnZip / CompZip / FindZip set it around their calls).
        "zip_legacy" = 1: zip_device_ex takes Shrink_1 and Reduce_1 .. _4, rezip_device the approaches shrink and reduce_4 (legacy=True sets it around the calls).
        "lzma_dict" is the reference's dictionary_size parameter for LZMA_3 (0 = the entry's size, what Zip.Compress.LZMA_E passes).
        "trained_fork" = 0: TrainedCompression works through every entry's whole stream (the same bytes; for measurements).
        "descr_lazy" = 0: Deflate_3's splitter builds every window's descriptor instead of only those a bound on the distance does not decide (the same bytes; for A/B and cross-checks).
        "match_first" = 0: k_match leaves every search's first candidate to the walker instead of settling it in the fetch (the same bytes; for A/B)."""
        if self.lib.zada_set_knob(self.ctx, name.encode(), int(value)) != 0:
            raise ZadaError("unknown knob %r" % name)
        self.__dict__.setdefault("_knobs_set", {})[name] = int(value)          # (what a caller that sets a knob around a call puts back)

    def _err(self, rc, what):
        if rc == E_DATA:
            raise DataError("%s: %s" % (what, self.lib.zada_last_error(self.ctx).decode()))
        if rc == E_REFERENCE:
            raise ReferenceDefect("%s: rc=%d (%s)" % (what, rc, self.lib.zada_last_error(self.ctx).decode()))
        raise ZadaError("%s failed: rc=%d (%s)" % (what, rc, self.lib.zada_last_error(self.ctx).decode()))

    def deflate(self, data, method=Method.Deflate_3, crc=0xFFFFFFFF, feedback=None):
        """Zip.Compress.Deflate.  Returns (raw deflate bytes, running CRC register).
        Raises CompressionInefficient when compression_ok would be False."""
        n = len(data)
        out = ctypes.create_string_buffer(n + 64)
        ol = ctypes.c_uint64(0)
        c = ctypes.c_uint32(crc)
        cb = FEEDBACK_FN(lambda pct, _u: 1 if feedback(pct) else 0) if feedback else None
        rc = self.lib.zada_deflate(self.ctx, method, _addr(data) if n else None, n, ctypes.addressof(out), n + 64,
                                   ctypes.byref(ol), ctypes.byref(c), ctypes.cast(cb, ctypes.c_void_p) if cb else None, None)
        if rc == 1:
            raise CompressionInefficient()
        if rc == 2:
            raise UserAbort()
        if rc != 0:
            self._err(rc, "zada_deflate")
        return out.raw[:ol.value], c.value

    def bzip2(self, data, method=14, crc=0xFFFFFFFF, feedback=None, cap=None):
        """Zip.Compress.BZip2_E (method 12 / 13 / 14 = BZip2_1 / _2 / _3).  Returns (rc, BZip2 stream, running CRC register);
        rc 1 = not smaller than the input (the stream is still returned when it fits `cap`, default len(data) * 5 // 4 + 4096)."""
        n = len(data)
        cap = int(cap if cap is not None else n + n // 4 + 4096)
        out = ctypes.create_string_buffer(cap)
        ol = ctypes.c_uint64(0)
        c = ctypes.c_uint32(crc)
        cb = FEEDBACK_FN(lambda pct, _u: 1 if feedback(pct) else 0) if feedback else None
        rc = self.lib.zada_bzip2(self.ctx, method, _addr(data) if n else None, n, ctypes.addressof(out), cap, ctypes.byref(ol), ctypes.byref(c),
                                 ctypes.cast(cb, ctypes.c_void_p) if cb else None, None)
        if rc == 2:
            raise UserAbort()
        if rc < 0:
            self._err(rc, "zada_bzip2")
        return rc, (out.raw[:ol.value] if ol.value <= cap else None), c.value

    def bzip2_batch(self, datas, method=14, crc=0xFFFFFFFF):
        """Independent BZip2 streams (one per Zip entry) in one call: zada_bzip2_batch takes the entries that are one block each
        (up to 0.8 block capacities) through ONE launch sequence.  Returns a list of (rc, stream or None, running CRC register);
        rc 1 = not smaller than the input (the stream is still there when it fits len + len // 4 + 1024 bytes)."""
        import numpy as np
        cnt = len(datas)
        if cnt == 0:
            return []
        lens = np.fromiter((len(d) for d in datas), dtype=np.uint64, count=cnt)
        caps = lens + lens // 4 + 1024
        offs = np.concatenate(([0], np.cumsum(caps)[:-1])).astype(np.uint64)
        arena = np.empty(int(caps.sum()), dtype=np.uint8)
        outp = (arena.ctypes.data + offs).astype(np.uint64)
        keep = [d if len(d) else b"\0" for d in datas]
        ins = np.fromiter((_addr(d) for d in keep), dtype=np.uint64, count=cnt)
        ols = np.zeros(cnt, dtype=np.uint64)
        crcs = np.full(cnt, crc, dtype=np.uint32)
        rcs = np.zeros(cnt, dtype=np.int32)
        worst = self.lib.zada_bzip2_batch(self.ctx, method, cnt, ins.ctypes.data, lens.ctypes.data, outp.ctypes.data, caps.ctypes.data,
                                          ols.ctypes.data, crcs.ctypes.data, rcs.ctypes.data)
        if worst < 0:
            self._err(worst, "zada_bzip2_batch")
        mv = memoryview(arena)
        return [(int(rcs[i]), bytes(mv[int(offs[i]):int(offs[i]) + int(ols[i])]) if rcs[i] >= 0 and ols[i] <= caps[i] else None, int(crcs[i])) for i in range(cnt)]

    def lzma(self, data, method=18, crc=0xFFFFFFFF, cap=None, feedback=None):
        """Zip.Compress.LZMA_E (method 15 .. 33 = LZMA_0 .. LZMA_for_AU, Method).  Returns (rc, Zip payload, running CRC register); rc 1 = not
        smaller than the input (the payload is still returned when it fits `cap`, default len(data) * 9 // 8 + 4096).
        feedback(percent) is called between the launches of the stream; a true return raises UserAbort."""
        n = len(data)
        cap = int(cap if cap is not None else n + n // 8 + 4096)
        out = ctypes.create_string_buffer(cap)
        ol = ctypes.c_uint64(0)
        c = ctypes.c_uint32(crc)
        cb = FEEDBACK_FN(lambda pct, _u: 1 if feedback(pct) else 0) if feedback else None
        rc = self.lib.zada_lzma(self.ctx, method, _addr(data) if n else None, n, ctypes.addressof(out), cap, ctypes.byref(ol), ctypes.byref(c),
                                ctypes.cast(cb, ctypes.c_void_p) if cb else None, None)
        if rc == 2:
            raise UserAbort()
        if rc < 0:
            self._err(rc, "zada_lzma")
        return rc, (out.raw[:ol.value] if ol.value <= cap else None), c.value

    def lzma_export_state(self, out_cap):
        """After lzma() raised UserAbort (its feedback stopped the stream between two launches): (state bytes, the stream bytes written so far,
        input positions coded).  zada_lzma_export_state."""
        sl = ctypes.c_uint64(0)
        self.lib.zada_lzma_export_state(self.ctx, None, 0, ctypes.byref(sl), None, 0, None, None)
        state = ctypes.create_string_buffer(sl.value)
        out = ctypes.create_string_buffer(int(out_cap))
        ob, pos = ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = self.lib.zada_lzma_export_state(self.ctx, ctypes.addressof(state), sl.value, ctypes.byref(sl), ctypes.addressof(out), int(out_cap), ctypes.byref(ob), ctypes.byref(pos))
        if rc != 0:
            self._err(rc, "zada_lzma_export_state")
        return state.raw[:sl.value], out.raw[:ob.value], pos.value

    def lzma_import_state(self, state):
        """The NEXT lzma() call of this encoder -- same input, same method -- goes on from `state` (lzma_export_state of any context or process); its
        payload is valid from the exported stream bytes' length on."""
        rc = self.lib.zada_lzma_import_state(self.ctx, _addr(state), len(state))
        if rc != 0:
            self._err(rc, "zada_lzma_import_state")

    def lzma_batch(self, datas, method=18, crc=0xFFFFFFFF):
        """Independent LZMA payloads (one per Zip entry; method 15 .. 33) in one call: every entry is a workgroup of ONE launch of the coder
        (methods whose literal table is in HBM: one launch per group of at most "lzma_lit_mib" MiB of tables).  Returns a list of (rc, payload or None, running CRC register)."""
        import numpy as np
        cnt = len(datas)
        if cnt == 0:
            return []
        lens = np.fromiter((len(d) for d in datas), dtype=np.uint64, count=cnt)
        caps = lens + lens // 8 + 128
        offs = np.concatenate(([0], np.cumsum(caps)[:-1])).astype(np.uint64)
        arena = np.empty(int(caps.sum()), dtype=np.uint8)
        outp = (arena.ctypes.data + offs).astype(np.uint64)
        keep = [d if len(d) else b"\0" for d in datas]
        ins = np.fromiter((_addr(d) for d in keep), dtype=np.uint64, count=cnt)
        ols = np.zeros(cnt, dtype=np.uint64)
        crcs = np.full(cnt, crc, dtype=np.uint32)
        rcs = np.zeros(cnt, dtype=np.int32)
        worst = self.lib.zada_lzma_batch(self.ctx, method, cnt, ins.ctypes.data, lens.ctypes.data, outp.ctypes.data, caps.ctypes.data,
                                         ols.ctypes.data, crcs.ctypes.data, rcs.ctypes.data)
        if worst < 0 and not (worst == E_REFERENCE and all(r >= 0 or r == E_REFERENCE for r in rcs)):     # (refused entries: rc -6, no payload)
            self._err(worst, "zada_lzma_batch")
        mv = memoryview(arena)
        return [(int(rcs[i]), bytes(mv[int(offs[i]):int(offs[i]) + int(ols[i])]) if rcs[i] >= 0 and ols[i] <= caps[i] else None, int(crcs[i])) for i in range(cnt)]

    # ---- Shrink_1 and Reduce_1 .. _4 (include/zada.h "Shrink_1 and Reduce_1 .. _4"): one wave per entry, so the batch calls are what fills the device ----
    def _legacy_one(self, data, method, crc, cap):
        n = len(data)
        cap = int(n if cap is None else cap)
        out = ctypes.create_string_buffer(max(cap, 1))
        ol = ctypes.c_uint64(0)
        c = ctypes.c_uint32(crc)
        if method == Method.Shrink_1:
            rc, who = self.lib.zada_shrink(self.ctx, _addr(data) if n else None, n, ctypes.addressof(out), cap, ctypes.byref(ol), ctypes.byref(c)), "zada_shrink"
        else:
            rc, who = self.lib.zada_reduce(self.ctx, method, _addr(data) if n else None, n, ctypes.addressof(out), cap, ctypes.byref(ol), ctypes.byref(c)), "zada_reduce"
        if rc < 0:
            self._err(rc, who)
        return rc, (out.raw[:ol.value] if rc == 0 else None), ol.value, c.value

    def shrink(self, data, crc=0xFFFFFFFF, cap=None):
        """Zip.Compress.Shrink_E (Shrink_1).  Returns (rc, stream or None, stream length, running CRC register); rc 1 = the stream is not shorter than
        the input and is not delivered.  cap defaults to len (data), which always suffices."""
        return self._legacy_one(data, Method.Shrink_1, crc, cap)

    def reduce(self, data, method=Method.Reduce_4, crc=0xFFFFFFFF, cap=None):
        """Zip.Compress.Reduce (method 2 .. 5 = Reduce_1 .. _4).  Returns as shrink ()."""
        return self._legacy_one(data, method, crc, cap)

    def _legacy_batch(self, datas, method, crc):
        import numpy as np
        cnt = len(datas)
        if cnt == 0:
            return []
        lens = np.fromiter((len(d) for d in datas), dtype=np.uint64, count=cnt)
        caps = lens.copy()
        offs = np.concatenate(([0], np.cumsum(caps)[:-1])).astype(np.uint64)
        arena = np.empty(int(caps.sum()) + 1, dtype=np.uint8)
        outp = (arena.ctypes.data + offs).astype(np.uint64)
        keep = [d if len(d) else b"\0" for d in datas]
        ins = np.fromiter((_addr(d) for d in keep), dtype=np.uint64, count=cnt)
        ols = np.zeros(cnt, dtype=np.uint64)
        crcs = np.full(cnt, crc, dtype=np.uint32)
        rcs = np.zeros(cnt, dtype=np.int32)
        if method == Method.Shrink_1:
            worst, who = self.lib.zada_shrink_batch(self.ctx, cnt, ins.ctypes.data, lens.ctypes.data, outp.ctypes.data, caps.ctypes.data, ols.ctypes.data,
                                                    crcs.ctypes.data, rcs.ctypes.data), "zada_shrink_batch"
        else:
            worst, who = self.lib.zada_reduce_batch(self.ctx, method, cnt, ins.ctypes.data, lens.ctypes.data, outp.ctypes.data, caps.ctypes.data, ols.ctypes.data,
                                                    crcs.ctypes.data, rcs.ctypes.data), "zada_reduce_batch"
        if worst < 0:
            self._err(worst, who)
        mv = memoryview(arena)
        return [(int(rcs[i]), bytes(mv[int(offs[i]):int(offs[i]) + int(ols[i])]) if rcs[i] == 0 else None, int(crcs[i])) for i in range(cnt)]

    def shrink_batch(self, datas, crc=0xFFFFFFFF):
        """Independent Shrink_1 streams (one per Zip entry) in one call, one wave per entry.  Returns a list of (rc, stream or None, running CRC
        register); rc 1: the stream is not shorter than the entry (Store it)."""
        return self._legacy_batch(datas, Method.Shrink_1, crc)

    def reduce_batch(self, datas, method=Method.Reduce_4, crc=0xFFFFFFFF):
        """Independent Reduce streams (method 2 .. 5) in one call, in launch groups bounded by the knob "reduce_group_mib".  Returns as shrink_batch ()."""
        return self._legacy_batch(datas, method, crc)

    def shrink_device(self, d_in, n, d_out, cap, crc=0xFFFFFFFF):
        """Shrink_1 stream of n bytes at device address d_in into d_out (cap bytes).  Returns (rc, length, running CRC register)."""
        ol = ctypes.c_uint64(0)
        c = ctypes.c_uint32(crc)
        rc = self.lib.zada_shrink_device(self.ctx, d_in, n, d_out, cap, ctypes.byref(ol), ctypes.byref(c))
        if rc < 0:
            self._err(rc, "zada_shrink_device")
        return rc, ol.value, c.value

    def reduce_device(self, d_in, n, d_out, cap, method=Method.Reduce_4, crc=0xFFFFFFFF):
        """Reduce stream (method 2 .. 5) of n bytes at device address d_in into d_out (cap bytes).  Returns (rc, length, running CRC register)."""
        ol = ctypes.c_uint64(0)
        c = ctypes.c_uint32(crc)
        rc = self.lib.zada_reduce_device(self.ctx, method, d_in, n, d_out, cap, ctypes.byref(ol), ctypes.byref(c))
        if rc < 0:
            self._err(rc, "zada_reduce_device")
        return rc, ol.value, c.value

    def reduce_last_record(self, entry=0):
        """Test hook (zada_reduce_last_record): what the last Reduce launch group left for its entry `entry`: (raw bytes, Slen [256] u8,
        followers [256, 32] u8)."""
        import numpy as np
        k = self.lib.zada_reduce_last_record(self.ctx, 0, entry, None, 0)
        raw = ctypes.create_string_buffer(max(int(k), 1))
        slen, foll = np.zeros(256, np.uint8), np.zeros((256, 32), np.uint8)
        self.lib.zada_reduce_last_record(self.ctx, 0, entry, ctypes.addressof(raw), k)
        if self.lib.zada_reduce_last_record(self.ctx, 1, entry, slen.ctypes.data, 256) != 256 or self.lib.zada_reduce_last_record(self.ctx, 2, entry, foll.ctypes.data, 8192) != 8192:
            raise ZadaError("zada_reduce_last_record: no such entry")
        return raw.raw[:k], slen, foll

    def lzma_match_sets(self, data, stride=50):
        """Test hook: the match sets of LZMA_3's BT4 matcher at every position of `data`, as the producer kernels leave them for the coder
        (lz77.adb:1234-1361).  Returns (cnt [n] u8, len [n, stride] u16, dist [n, stride] u32)."""
        import numpy as np
        n = len(data)
        cnt = np.zeros(n, np.uint8); ln = np.zeros((n, stride), np.uint16); ds = np.zeros((n, stride), np.uint32)
        rc = self.lib.zada_lzma_match_sets(self.ctx, _addr(data) if n else None, n, cnt.ctypes.data, ln.ctypes.data, ds.ctypes.data, stride)
        if rc < 0:
            self._err(rc, "zada_lzma_match_sets")
        return cnt, ln, ds

    def lzma_device(self, d_in, n, d_out, cap, method=18, crc=0xFFFFFFFF):
        """LZMA payload of n bytes at device address d_in into d_out (cap bytes).  Returns (rc, length, running CRC register)."""
        ol = ctypes.c_uint64(0)
        c = ctypes.c_uint32(crc)
        rc = self.lib.zada_lzma_device(self.ctx, method, d_in, n, d_out, cap, ctypes.byref(ol), ctypes.byref(c))
        if rc < 0:
            self._err(rc, "zada_lzma_device")
        return rc, ol.value, c.value

    def bzip2_device(self, d_in, n, d_out, cap, method=14, crc=0xFFFFFFFF):
        """BZip2 stream of n bytes at device address d_in into d_out (cap bytes).  Returns (rc, length, running CRC register)."""
        ol = ctypes.c_uint64(0)
        c = ctypes.c_uint32(crc)
        rc = self.lib.zada_bzip2_device(self.ctx, method, d_in, n, d_out, cap, ctypes.byref(ol), ctypes.byref(c))
        if rc < 0:
            self._err(rc, "zada_bzip2_device")
        return rc, ol.value, c.value

    def crc32_device(self, d_ptr, n):
        """Raw CRC-32 register (started from 0) of n bytes at a 16-byte aligned device address (see crc32_combine)."""
        raw = ctypes.c_uint32(0)
        rc = self.lib.zada_crc32_device(self.ctx, d_ptr, n, ctypes.byref(raw))
        if rc != 0:
            self._err(rc, "zada_crc32_device")
        return raw.value

    # ---- one BZip2 stream over several contexts (zada_bz2_range_*, include/zada.h) ----
    def bz2_range_open(self, d_buf, buf_len, buf_off, stream_total, start, own_end, method=14):
        """Block limits of the blocks that start in [start, own_end).  Returns (next_start, number of blocks)."""
        nxt, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = self.lib.zada_bz2_range_open(self.ctx, method, d_buf, buf_len, buf_off, stream_total, start, own_end, ctypes.byref(nxt), ctypes.byref(nb))
        if rc != 0:
            self._err(rc, "zada_bz2_range_open")
        return nxt.value, nb.value

    def bz2_range_encode(self):
        rc = self.lib.zada_bz2_range_encode(self.ctx)
        if rc != 0:
            self._err(rc, "zada_bz2_range_encode")

    def bz2_range_table(self):
        """numpy uint64 [blocks, 4 tactics, 3]: bits (all ones: the block has no such tactic), pieces, folded CRC."""
        import numpy as np
        nb = self.lib.zada_bz2_range_table(self.ctx, None, 0)
        tab = np.zeros((max(int(nb), 1), 4, 3), np.uint64)
        self.lib.zada_bz2_range_table(self.ctx, tab.ctypes.data, nb)
        return tab[:nb]

    def bz2_select(self, tab, bitpos_in=32, crc_in=0):
        """Tactic per block along the stream.  Returns (choices uint8 array, bit position behind, combined CRC behind)."""
        import numpy as np
        tab = np.ascontiguousarray(tab, np.uint64)
        nb = tab.shape[0]
        choice = np.zeros(max(nb, 1), np.uint8)
        bp, crc = ctypes.c_uint64(0), ctypes.c_uint32(0)
        self.lib.zada_bz2_select(nb, tab.ctypes.data, bitpos_in, crc_in, choice.ctypes.data, ctypes.byref(bp), ctypes.byref(crc))
        return choice[:nb], bp.value, crc.value

    def bz2_range_assemble(self, choice, bit_begin, d_out, cap, header=False, footer_crc=None):
        """The range's bytes of the stream (from byte bit_begin // 8 on) into d_out.  Returns their number."""
        import numpy as np
        choice = np.ascontiguousarray(choice, np.uint8)
        nbytes = ctypes.c_uint64(0)
        flags = (1 if header else 0) | (2 if footer_crc is not None else 0)
        rc = self.lib.zada_bz2_range_assemble(self.ctx, choice.ctypes.data if len(choice) else None, len(choice), bit_begin, flags, footer_crc or 0, d_out, cap, ctypes.byref(nbytes))
        if rc != 0:
            self._err(rc, "zada_bz2_range_assemble")
        return nbytes.value

    def bz2_last_blocks(self):
        """[(raw start, raw length, tactic, sub-blocks)] of the last bzip2 call (bzip2-encoding.adb:1144, :1312-1318)."""
        import numpy as np
        k = self.lib.zada_bz2_last_blocks(self.ctx, None, 0)
        buf = np.zeros(max(int(k), 1), np.uint64)
        self.lib.zada_bz2_last_blocks(self.ctx, buf.ctypes.data, k)
        return [tuple(int(x) for x in buf[i:i + 4]) for i in range(0, int(k), 4)]

    def deflate_into(self, data, out, method=Method.Deflate_3, crc=0xFFFFFFFF):
        """Zip.Compress.Deflate into a caller-owned buffer (bytearray / numpy uint8 / ctypes, len(out) >= len(data) + 64):
        no allocation on the way.  Returns (rc, out_len, running CRC register); rc 1 = inefficient."""
        n = len(data)
        ol = ctypes.c_uint64(0)
        c = ctypes.c_uint32(crc)
        rc = self.lib.zada_deflate(self.ctx, method, _addr(data) if n else None, n, _addr(out), len(out), ctypes.byref(ol), ctypes.byref(c), None, None)
        if rc < 0 or rc == 2:
            self._err(rc, "zada_deflate")
        return rc, ol.value, c.value

    def deflate_batch(self, datas, method=Method.Deflate_3, crc=0xFFFFFFFF):
        """Independent streams (one per Zip entry, Zip.Create.Add_Stream is per entry) in one call: zada_deflate_batch takes
        the entries of up to 4 MiB through ONE launch sequence.  Returns a list of (rc, raw deflate bytes or None, running
        CRC register); rc 1 = inefficient (the caller Stores the entry)."""
        import numpy as np
        cnt = len(datas)
        if cnt == 0:
            return []
        lens = np.fromiter((len(d) for d in datas), dtype=np.uint64, count=cnt)
        caps = lens + 64
        offs = np.concatenate(([0], np.cumsum(caps)[:-1])).astype(np.uint64)
        arena = np.empty(int(caps.sum()), dtype=np.uint8)                       # one output arena instead of one buffer per entry
        outp = (arena.ctypes.data + offs).astype(np.uint64)
        keep = [d if len(d) else b"\0" for d in datas]
        ins = np.fromiter((_addr(d) for d in keep), dtype=np.uint64, count=cnt)
        ols = np.zeros(cnt, dtype=np.uint64)
        crcs = np.full(cnt, crc, dtype=np.uint32)
        rcs = np.zeros(cnt, dtype=np.int32)
        worst = self.lib.zada_deflate_batch(self.ctx, method, cnt, ins.ctypes.data, lens.ctypes.data, outp.ctypes.data, caps.ctypes.data,
                                            ols.ctypes.data, crcs.ctypes.data, rcs.ctypes.data)
        if worst < 0:
            self._err(worst, "zada_deflate_batch")
        mv = memoryview(arena)
        return [(int(rcs[i]), bytes(mv[int(offs[i]):int(offs[i]) + int(ols[i])]) if rcs[i] == 0 else None, int(crcs[i])) for i in range(cnt)]

    def deflate_device(self, d_in_ptr, n, d_out_ptr, cap, method=Method.Deflate_3, crc=0xFFFFFFFF):
        """Device-resident variant (pointers are HBM addresses, e.g. torch tensor .data_ptr()).
        Returns (rc, out_len, crc); rc 1 = inefficient."""
        ol = ctypes.c_uint64(0)
        c = ctypes.c_uint32(crc)
        rc = self.lib.zada_deflate_device(self.ctx, method, d_in_ptr, n, d_out_ptr, cap, ctypes.byref(ol), ctypes.byref(c))
        if rc < 0:
            self._err(rc, "zada_deflate_device")
        return rc, ol.value, c.value

    def compress_data(self, data, method=Method.Deflate_3, content_hint=None, password=None, header=None):
        """Zip.Compress.Compress_Data: returns (payload bytes, final CRC-32, zip_type) with the Store fallback applied.
        With a content_hint (ContentType) the method may be a Preselection method: the entry's method is then chosen by the content hint
        and len(data) (zada_compress_data_hint, preselect).  Without one, a single method.
        With a password (bytes, or str taken as Latin-1) the payload is the 12-byte encryption header followed by the encoded stream
        (zada_compress_data_pw); `header` holds the header's eleven random bytes (default: os.urandom (11))."""
        n = len(data)
        if password is not None:
            pw = _password(password)
            h11 = os.urandom(11) if header is None else bytes(header)
            if len(h11) != 11:
                raise ZadaError("header: eleven bytes")
            out = ctypes.create_string_buffer(n + 64 + 12)
            ol, c, zt = ctypes.c_uint64(0), ctypes.c_uint32(0), ctypes.c_uint16(0)
            rc = self.lib.zada_compress_data_pw(self.ctx, method, ContentType.neutral if content_hint is None else int(content_hint), pw, len(pw), h11,
                                                _addr(data) if n else None, n, ctypes.addressof(out), n + 64 + 12, ctypes.byref(ol), ctypes.byref(c), ctypes.byref(zt), None)
            if rc != 0:
                self._err(rc, "zada_compress_data_pw")
            return out.raw[:ol.value], c.value, zt.value
        if method == Method.Store:
            import zlib  # CRC of stored data only; not on the Deflate path
            return bytes(data), zlib.crc32(data) & 0xFFFFFFFF, 0
        out = ctypes.create_string_buffer(n + 64)
        ol = ctypes.c_uint64(0)
        c = ctypes.c_uint32(0)
        zt = ctypes.c_uint16(0)
        if content_hint is None:
            rc = self.lib.zada_compress_data(self.ctx, method, _addr(data) if n else None, n, ctypes.addressof(out), n + 64,
                                             ctypes.byref(ol), ctypes.byref(c), ctypes.byref(zt))
        else:
            rc = self.lib.zada_compress_data_hint(self.ctx, method, int(content_hint), _addr(data) if n else None, n, ctypes.addressof(out), n + 64,
                                                  ctypes.byref(ol), ctypes.byref(c), ctypes.byref(zt), None)
        if rc != 0:
            self._err(rc, "zada_compress_data")
        return out.raw[:ol.value], c.value, zt.value

    # ---- ZipCrypto (Zip.CRC_Crypto, zip-crc_crypto.adb:78-137; include/zada.h "Password-protected entries") ----
    def crypt_init_keys(self, password):
        """Init_Keys: the three keys of a password (bytes, or str taken as Latin-1)."""
        pw = password.encode("latin-1") if isinstance(password, str) else bytes(password)
        k = (ctypes.c_uint32 * 3)()
        self.lib.zada_crypt_init_keys(pw, len(pw), k)
        return tuple(k)

    def crypt_header(self, keys, random11, crc_final):
        """The encryption header (zip-compress.adb:153-161) of eleven bytes and the entry's final CRC-32: (12 encoded bytes, keys behind them)."""
        if len(random11) != 11:
            raise ZadaError("header: eleven bytes")
        k = (ctypes.c_uint32 * 3)(*keys)
        out = ctypes.create_string_buffer(12)
        self.lib.zada_crypt_header(k, bytes(random11), crc_final & 0xFFFFFFFF, ctypes.addressof(out))
        return out.raw, tuple(k)

    def crypt_encode(self, keys, data):
        """Encode of `data` from `keys`: (cipher text, keys behind it).  Piece after piece gives the bytes of one call over the whole."""
        import numpy as np
        k = (ctypes.c_uint32 * 3)(*keys)
        buf = np.frombuffer(data, dtype=np.uint8).copy() if len(data) else np.zeros(0, np.uint8)
        rc = self.lib.zada_crypt_encode(self.ctx, k, buf.ctypes.data if len(buf) else None, len(buf))
        if rc != 0:
            self._err(rc, "zada_crypt_encode")
        return buf.tobytes(), tuple(k)

    def crypt_encode_device(self, keys, d_ptr, n):
        """Encode of n bytes at a device address, in place.  Returns the keys behind them."""
        k = (ctypes.c_uint32 * 3)(*keys)
        rc = self.lib.zada_crypt_encode_device(self.ctx, k, d_ptr, n)
        if rc != 0:
            self._err(rc, "zada_crypt_encode_device")
        return tuple(k)

    def crypt_encode_batch(self, keys, datas):
        """Independent buffers, each from its own keys, in one call (zada_crypt_encode_batch).  Returns a list of (cipher text, keys behind it)."""
        import numpy as np
        cnt = len(datas)
        if cnt == 0:
            return []
        lens = np.fromiter((len(d) for d in datas), dtype=np.uint64, count=cnt)
        offs = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.uint64)
        arena = np.frombuffer(b"".join(bytes(d) for d in datas) or b"\0", dtype=np.uint8).copy()
        ptrs = (arena.ctypes.data + offs).astype(np.uint64)
        ks = np.ascontiguousarray(np.array(keys, dtype=np.uint32).reshape(cnt, 3))
        rc = self.lib.zada_crypt_encode_batch(self.ctx, cnt, ks.ctypes.data, ptrs.ctypes.data, lens.ctypes.data)
        if rc != 0:
            self._err(rc, "zada_crypt_encode_batch")
        mv = memoryview(arena)
        return [(bytes(mv[int(offs[i]):int(offs[i]) + int(lens[i])]), tuple(int(x) for x in ks[i])) for i in range(cnt)]

    def crypt_decode_batch(self, keys, datas):
        """Decode (zip-crc_crypto.adb:130-137) of independent buffers, each from its own keys, in one launch (zada_crypt_decode_batch: one lane per
        buffer -- Decode is serial).  Returns a list of (plain text, keys behind it)."""
        import numpy as np
        cnt = len(datas)
        if cnt == 0:
            return []
        lens = np.fromiter((len(d) for d in datas), dtype=np.uint64, count=cnt)
        offs = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.uint64)
        arena = np.frombuffer(b"".join(bytes(d) for d in datas) or b"\0", dtype=np.uint8).copy()
        ptrs = (arena.ctypes.data + offs).astype(np.uint64)
        ks = np.ascontiguousarray(np.array(keys, dtype=np.uint32).reshape(cnt, 3))
        rc = self.lib.zada_crypt_decode_batch(self.ctx, cnt, ks.ctypes.data, ptrs.ctypes.data, lens.ctypes.data)
        if rc != 0:
            self._err(rc, "zada_crypt_decode_batch")
        mv = memoryview(arena)
        return [(bytes(mv[int(offs[i]):int(offs[i]) + int(lens[i])]), tuple(int(x) for x in ks[i])) for i in range(cnt)]

    # ---- what the methods of the four readers share: fn is the entry point of the C ABI, `lead` its arguments in front of the stream, `mid` those
    # between cap and out_len; `who` its name in the error texts ----
    def _reader_single(self, fn, who, payload, cap, crc, grow, lead=(), mid=()):
        """One stream on host buffers.  grow: the cap doubles while the only complaint is "output beyond cap"."""
        n = len(payload)
        while True:
            out = ctypes.create_string_buffer(max(cap, 1))
            ol, iu, c = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(crc)
            rc = fn(self.ctx, *lead, _addr(payload) if n else None, n, ctypes.addressof(out), cap, *mid, ctypes.byref(ol), ctypes.byref(iu), ctypes.byref(c))
            if rc == 0:
                return out.raw[:ol.value], iu.value, c.value
            if rc == E_DATA and grow and b"output beyond cap" in self.lib.zada_last_error(self.ctx):
                cap *= 2
                continue
            self._err(rc, who)

    def _reader_device(self, fn, who, d_in_ptr, n_in, d_out_ptr, cap, crc, lead=(), mid=()):
        ol, iu, c = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(crc)
        rc = fn(self.ctx, *lead, d_in_ptr, n_in, d_out_ptr, cap, *mid, ctypes.byref(ol), ctypes.byref(iu), ctypes.byref(c))
        if rc != 0:
            self._err(rc, who)
        return ol.value, iu.value, c.value

    def _reader_batch(self, who, payloads, caps, crc, deliver, call):
        """caps: one per payload, as a contiguous numpy array of 64-bit values.  call (count, in pointers, lengths, out pointers or None, caps, out_len,
        in_used, crc, rc): the batch call of the C ABI on the addresses of these arrays, with the format's own arrays spliced in."""
        import numpy as np
        cnt = len(payloads)
        lens = np.fromiter((len(d) for d in payloads), dtype=np.uint64, count=cnt)
        keep = [d if len(d) else b"\0" for d in payloads]
        ins = np.fromiter((_addr(d) for d in keep), dtype=np.uint64, count=cnt)
        total = sum(int(x) for x in caps)                  # (Python integers: the sizes may come from a directory that lies)
        try:
            if total >= 1 << 40:
                raise MemoryError
            arena = np.empty(total + 1 if deliver else 1, dtype=np.uint8)
        except (MemoryError, ValueError):
            raise ZadaError("%s: %d bytes of output are promised -- more than this machine holds" % (who, total))
        offs = np.concatenate(([0], np.cumsum(caps)[:-1])).astype(np.uint64)
        outp = (arena.ctypes.data + offs).astype(np.uint64)
        ols, ius = np.zeros(cnt, dtype=np.uint64), np.zeros(cnt, dtype=np.uint64)
        crcs = np.full(cnt, crc, dtype=np.uint32)
        rcs = np.zeros(cnt, dtype=np.int32)
        worst = call(cnt, ins.ctypes.data, lens.ctypes.data, outp.ctypes.data if deliver else None, caps.ctypes.data, ols.ctypes.data, ius.ctypes.data,
                     crcs.ctypes.data, rcs.ctypes.data)
        if worst < 0 and worst != E_DATA:
            self._err(worst, "zada_" + who)
        mv = memoryview(arena)
        return [(int(rcs[i]), bytes(mv[int(offs[i]):int(offs[i]) + int(ols[i])]) if deliver and rcs[i] == 0 else None, int(ols[i]), int(ius[i]), int(crcs[i]))
                for i in range(cnt)]

    def _reader_last_records(self, fn, width, *lead):
        import numpy as np
        n = fn(self.ctx, *lead, None, 0)
        a = np.zeros(max(int(n), 1), dtype=np.uint64)
        fn(self.ctx, *lead, a.ctypes.data, int(n))
        return a[:int(n)].reshape(-1, width)

    # ---- the reader: UnZip.Decompress.Inflate (unzip-decompress.adb:1463-1889; include/zada.h "Inflate") ----
    def inflate(self, payload, size=None, format=8, crc=0xFFFFFFFF):
        """One raw Deflate (format 8) or Deflate64 (9) stream.  size: the uncompressed size the directory promises (a stream that writes more is a
        DataError); None = unknown: the output buffer starts at four times the payload and doubles while the only complaint is "output beyond cap".
        Returns (bytes, input bytes used, running CRC register).  Raises DataError."""
        cap = max(4 * len(payload), 256) if size is None else int(size)
        return self._reader_single(self.lib.zada_inflate, "zada_inflate", payload, cap, crc, size is None, lead=(format,))

    def inflate_batch(self, payloads, sizes, formats=8, crc=0xFFFFFFFF, deliver=True):
        """Independent streams (one per Zip entry), one wave each, in one launch per group of "batch_mib".  sizes [i] = cap of entry i; formats: one
        Zip code for all, or one per entry.  Returns a list of (rc, bytes or None, bytes written, input bytes used, running CRC register); rc is 0
        or E_DATA.  deliver = False: the bytes stay on the device (sizes and CRCs only -- UnZip's test_only)."""
        import numpy as np
        cnt = len(payloads)
        if cnt == 0:
            return []
        fm = np.full(cnt, formats, dtype=np.int32) if np.isscalar(formats) else np.ascontiguousarray(np.array(formats, dtype=np.int32))
        caps = np.ascontiguousarray(np.array(sizes, dtype=np.uint64))
        if len(caps) != cnt or len(fm) != cnt:
            raise ZadaError("inflate_batch: one size and one format per payload")
        return self._reader_batch("inflate_batch", payloads, caps, crc, deliver,
                                  lambda cnt, ins, lens, *rest: self.lib.zada_inflate_batch(self.ctx, cnt, fm.ctypes.data, ins, lens, *rest))

    def inflate_device(self, d_in_ptr, n_in, d_out_ptr, cap, format=8, crc=0xFFFFFFFF):
        """Device-resident variant (HBM addresses of any alignment).  Returns (bytes written, input bytes used, running CRC register); raises DataError."""
        return self._reader_device(self.lib.zada_inflate_device, "zada_inflate_device", d_in_ptr, n_in, d_out_ptr, cap, crc, lead=(format,))

    # ---- one large Deflate stream on many waves (include/zada.h "One large Deflate stream"; experimental) ----
    INFLATE_PAR_REASONS = ("none", "damaged", "repairs", "single chunk", "format", "memory")

    def inflate_par(self, payload, size, format=8, crc=0xFFFFFFFF):
        """inflate (payload, size) with the stream cut into chunks of "inflate_par_chunk_kib", a wave per chunk (zada_inflate_par): the same
        result and the same DataError.  size is the cap, as the directory promises it.  Returns (bytes, input bytes used, running CRC register);
        inflate_par_last () says whether the stream ran that way."""
        n, cap = len(payload), int(size)
        out = ctypes.create_string_buffer(max(cap, 1))
        ol, iu, c = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(crc)
        rc = self.lib.zada_inflate_par(self.ctx, format, _addr(payload) if n else None, n, ctypes.addressof(out), cap, ctypes.byref(ol), ctypes.byref(iu), ctypes.byref(c))
        if rc != 0:
            self._err(rc, "zada_inflate_par")
        return out.raw[:ol.value], iu.value, c.value

    def inflate_par_device(self, d_in_ptr, n_in, d_out_ptr, cap, format=8, crc=0xFFFFFFFF):
        """inflate_device on many waves (zada_inflate_par_device).  Returns (bytes written, input bytes used, running CRC register); raises DataError."""
        ol, iu, c = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(crc)
        rc = self.lib.zada_inflate_par_device(self.ctx, format, d_in_ptr, n_in, d_out_ptr, cap, ctypes.byref(ol), ctypes.byref(iu), ctypes.byref(c))
        if rc != 0:
            self._err(rc, "zada_inflate_par_device")
        return ol.value, iu.value, c.value

    def inflate_par_last(self):
        """The record of the last inflate_par* call (or of the last unzip_device call with "inflate_par_min_kib" set, summed over its large entries):
        dict of chunks, live_chunks, repairs, scout_rounds, marker_bytes, fell_back, reason (a word of INFLATE_PAR_REASONS), streams."""
        import numpy as np
        r = np.zeros(1, dtype=np.dtype([("chunks", "<u8"), ("live_chunks", "<u8"), ("repairs", "<u8"), ("scout_rounds", "<u8"), ("marker_bytes", "<u8"),
                                        ("fell_back", "<i4"), ("reason", "<i4"), ("streams", "<u8")]))
        rc = self.lib.zada_inflate_par_last(self.ctx, r.ctypes.data)
        if rc != 0:
            self._err(rc, "zada_inflate_par_last")
        d = {k: int(r[k][0]) for k in r.dtype.names}
        d["reason"] = self.INFLATE_PAR_REASONS[d["reason"]]
        return d

    # ---- the reader: BZip2.Decoding.Decompress (bzip2-decoding.adb; include/zada.h "BZip2.Decoding") ----
    def bunzip2(self, payload, size=None, crc=0xFFFFFFFF):
        """One BZip2 stream (Zip format 12), its blocks in parallel.  size: the uncompressed size the directory promises (a stream that writes more
        is a DataError); None = unknown: the output buffer starts at eight times the payload and doubles while the only complaint is "output beyond
        cap".  Returns (bytes, input bytes used, running CRC register).  Raises DataError."""
        cap = max(8 * len(payload), 4096) if size is None else int(size)
        return self._reader_single(self.lib.zada_bunzip2, "zada_bunzip2", payload, cap, crc, size is None)

    def bunzip2_batch(self, payloads, sizes, crc=0xFFFFFFFF, deliver=True):
        """Independent BZip2 streams (one per Zip entry): the blocks of all of them through the same launches, in groups bounded by
        "bunzip_batch_mib".  sizes [i] = cap of entry i.  Returns a list of (rc, bytes or None, bytes written, input bytes used, running CRC
        register); rc is 0 or E_DATA.  deliver = False: the bytes stay on the device (sizes and CRCs only -- UnZip's test_only)."""
        import numpy as np
        cnt = len(payloads)
        if cnt == 0:
            return []
        caps = np.ascontiguousarray(np.array(sizes, dtype=np.uint64))
        if len(caps) != cnt:
            raise ZadaError("bunzip2_batch: one size per payload")
        return self._reader_batch("bunzip2_batch", payloads, caps, crc, deliver, lambda *a: self.lib.zada_bunzip2_batch(self.ctx, *a))

    def bunzip2_last_records(self, blocks=False):
        """The last bunzip2* call: per entry (rule, block, bit, 0) -- or, blocks = True, per block of the chains (entry, symbols, origin, stored CRC,
        end bit) -- as a numpy array of 64-bit values."""
        return self._reader_last_records(self.lib.zada_bunzip2_last_records, 5 if blocks else 4, int(blocks))

    def bunzip2_device(self, d_in_ptr, n_in, d_out_ptr, cap, crc=0xFFFFFFFF):
        """Device-resident variant (HBM addresses of any alignment).  Returns (bytes written, input bytes used, running CRC register); raises DataError."""
        return self._reader_device(self.lib.zada_bunzip2_device, "zada_bunzip2_device", d_in_ptr, n_in, d_out_ptr, cap, crc)

    # ---- the reader: LZMA.Decoding.Decode (lzma-decoding.adb; include/zada.h "LZMA.Decoding") ----
    def unlzma(self, payload, cap=None, eos=True, crc=0xFFFFFFFF):
        """One LZMA payload (Zip format 14: version, properties size, properties, range-coded stream).  cap: the uncompressed size the directory
        promises (a stream that writes more is a DataError; one without marker, eos = False, ends there); None = unknown (eos = True only): the
        output buffer starts at eight times the payload and doubles while the only complaint is "output beyond cap".  eos: bit 1 of the entry's
        general-purpose flags -- the stream ends on a marker.  Returns (bytes, input bytes used, running CRC register).  Raises DataError."""
        if cap is None and not eos:
            raise ZadaError("unlzma: a stream without marker needs its size")
        size, cap = cap, (max(8 * len(payload), 4096) if cap is None else int(cap))
        return self._reader_single(self.lib.zada_unlzma, "zada_unlzma", payload, cap, crc, size is None, mid=(int(bool(eos)),))

    def unlzma_batch(self, payloads, caps, eos=True, crc=0xFFFFFFFF, deliver=True):
        """Independent LZMA payloads (one per Zip entry), one wave per entry, in groups bounded by "batch_mib" (and, for literal tables in HBM,
        "lzma_lit_mib").  caps [i] = cap of entry i; eos: one flag for all, or one per entry.  Returns a list of (rc, bytes or None, bytes written,
        input bytes used, running CRC register); rc is 0 or E_DATA.  deliver = False: the bytes stay on the device (UnZip's test_only)."""
        import numpy as np
        cnt = len(payloads)
        if cnt == 0:
            return []
        caps = np.ascontiguousarray(np.array(caps, dtype=np.uint64))
        if len(caps) != cnt:
            raise ZadaError("unlzma_batch: one cap per payload")
        flags = np.full(cnt, int(bool(eos)), dtype=np.int32) if isinstance(eos, (bool, int)) else np.ascontiguousarray(np.array([int(bool(x)) for x in eos], dtype=np.int32))
        if len(flags) != cnt:
            raise ZadaError("unlzma_batch: one eos flag per payload")
        return self._reader_batch("unlzma_batch", payloads, caps, crc, deliver,
                                  lambda cnt, ins, lens, outp, caps, *rest: self.lib.zada_unlzma_batch(self.ctx, cnt, ins, lens, outp, caps, flags.ctypes.data, *rest))

    def unlzma_last_records(self):
        """The last unlzma* call: per entry (rule broken or 0, input byte, output position, how the stream ended -- 1: on a marker, 2: without, 0: it did
        not) as a numpy array of 64-bit values."""
        return self._reader_last_records(self.lib.zada_unlzma_last_records, 4)

    def unlzma_device(self, d_in_ptr, n_in, d_out_ptr, cap, eos=True, crc=0xFFFFFFFF):
        """Device-resident variant (HBM addresses of any alignment).  Returns (bytes written, input bytes used, running CRC register); raises DataError."""
        return self._reader_device(self.lib.zada_unlzma_device, "zada_unlzma_device", d_in_ptr, n_in, d_out_ptr, cap, crc, mid=(int(bool(eos)),))

    # ---- the reader: Unshrink, Unreduce, Explode (unzip-decompress.adb:590-1418; include/zada.h "Unshrink, Unreduce and Explode") ----
    def unlegacy(self, payload, cap, method, flags=0, crc=0xFFFFFFFF):
        """One Shrink (method 1), Reduce (2 .. 5) or Implode (6) payload.  cap: the uncompressed size the directory promises -- the stream ends when cap
        bytes are out, none of the formats has an end code.  flags: the entry's general-purpose flags (Implode: bit 1 = 8 KiB dictionary, bit 2 = three
        trees).  Returns (bytes, input bytes used, running CRC register).  Raises DataError."""
        return self._reader_single(self.lib.zada_unlegacy, "zada_unlegacy", payload, int(cap), crc, False, lead=(int(method), int(flags)))

    def unlegacy_batch(self, streams, caps, methods, flags=None, crc=0xFFFFFFFF, deliver=True):
        """Independent Shrink / Reduce / Implode payloads (one per Zip entry), one wave per entry, in groups bounded by "batch_mib"; one batch may mix
        methods (one launch per format present).  caps [i], methods [i] per entry (methods: one for all, or one per entry); flags: None, one value
        for all, or one per entry.  Returns a list of (rc, bytes or None, bytes written, input bytes used, running CRC register); rc is 0 or E_DATA.
        deliver = False: the bytes stay on the device (UnZip's test_only)."""
        import numpy as np
        cnt = len(streams)
        if cnt == 0:
            return []
        caps = np.ascontiguousarray(np.array(caps, dtype=np.uint64))
        if len(caps) != cnt:
            raise ZadaError("unlegacy_batch: one cap per stream")
        meth = np.full(cnt, int(methods), dtype=np.uint16) if isinstance(methods, int) else np.ascontiguousarray(np.array([int(m) for m in methods], dtype=np.uint16))
        flg = (np.full(cnt, 0 if flags is None else int(flags) & 0xFF, dtype=np.uint8) if flags is None or isinstance(flags, int)
               else np.ascontiguousarray(np.array([int(f) & 0xFF for f in flags], dtype=np.uint8)))
        if len(meth) != cnt or len(flg) != cnt:
            raise ZadaError("unlegacy_batch: one method and one flags value per stream")
        return self._reader_batch("unlegacy_batch", streams, caps, crc, deliver,
                                  lambda cnt, ins, lens, outp, caps, *rest: self.lib.zada_unlegacy_batch(self.ctx, cnt, ins, lens, outp, caps, meth.ctypes.data,
                                                                                                     flg.ctypes.data, *rest))

    def unlegacy_last_records(self):
        """The last unlegacy* call: per entry (rule broken or 0, input byte, output position, 0) as a numpy array of 64-bit values."""
        return self._reader_last_records(self.lib.zada_unlegacy_last_records, 4)

    def unlegacy_device(self, d_in_ptr, n_in, d_out_ptr, cap, method, flags=0, crc=0xFFFFFFFF):
        """Device-resident variant (HBM addresses of any alignment).  Returns (bytes written, input bytes used, running CRC register); raises DataError."""
        return self._reader_device(self.lib.zada_unlegacy_device, "zada_unlegacy_device", d_in_ptr, n_in, d_out_ptr, cap, crc, lead=(int(method), int(flags)))

    # ---- the archive reader on device memory (include/zada.h "an archive that lies in device memory") ----
    @staticmethod
    def unzip_dtypes():
        """(dtype of zada_unzip_entry, dtype of zada_unzip_result) as numpy structured types."""
        import numpy as np
        return (np.dtype([("in_off", "<u8"), ("n_in", "<u8"), ("out_off", "<u8"), ("cap", "<u8"), ("method", "<u2"), ("flags", "u1"), ("check", "u1"), ("pad", "<u4")]),
                np.dtype([("rc", "<i4"), ("crc", "<u4"), ("out_len", "<u8"), ("in_used", "<u8")]))

    def unzip_device(self, d_archive_ptr, archive_len, d_out_ptr, out_bytes, entries, keys0=None, crc=0xFFFFFFFF):
        """zada_unzip_device: `entries` is a numpy structured array of unzip_dtypes () [0] rows, keys0 the keys of the password (crypt_init_keys) or None,
        crc the running register the entries start from (one value or one per entry); d_out_ptr = None is the test-only form.  Returns (the call's return
        value -- the worst per-entry rc: 0, E_DATA or E_PASSWORD --, the structured array of results).  An argument the call refuses raises ZadaError."""
        import numpy as np
        dt_e, dt_r = self.unzip_dtypes()
        ent = np.ascontiguousarray(entries, dtype=dt_e)
        res = np.zeros(len(ent), dtype=dt_r)
        res["crc"] = crc
        k = (ctypes.c_uint32 * 3)(*keys0) if keys0 is not None else None
        rc = self.lib.zada_unzip_device(self.ctx, d_archive_ptr, archive_len, d_out_ptr, out_bytes, len(ent), ent.ctypes.data if len(ent) else None, k,
                                        res.ctypes.data if len(ent) else None)
        if rc not in (0, E_DATA, E_PASSWORD):
            self._err(rc, "zada_unzip_device")
        return rc, res

    # ---- the archive writer on device memory (include/zada.h "an archive made from entries in device memory") ----
    @staticmethod
    def zip_dtypes():
        """(dtype of zada_zip_entry, dtype of zada_zip_result) as numpy structured types."""
        import numpy as np
        return (np.dtype([("d_data", "<u8"), ("n", "<u8"), ("name", "<u8"), ("name_len", "<u4"), ("time", "<u4"), ("flags", "<u4"), ("pad", "<u4")]),
                np.dtype([("rc", "<i4"), ("zip_type", "<u2"), ("pad", "<u2"), ("crc", "<u4"), ("pad2", "<u4"), ("csize", "<u8"), ("offset", "<u8")]))

    def zip_bound(self, entries, archive_base=0):
        """zada_zip_bound: an upper bound on the archive zip_device makes of `entries` (only n and name_len are read)."""
        import numpy as np
        ent = np.ascontiguousarray(entries, dtype=self.zip_dtypes()[0])
        return int(self.lib.zada_zip_bound(len(ent), ent.ctypes.data if len(ent) else None, archive_base))

    def zip_device(self, entries, d_archive_ptr, cap, method=Method.Deflate_3, archive_base=0):
        """zada_zip_device: `entries` is a numpy structured array of zip_dtypes () [0] rows (d_data: device addresses; name: HOST addresses the caller keeps
        alive).  Returns (the archive's length, the structured array of results).  Whatever the call refuses raises ZadaError."""
        import numpy as np
        dt_e, dt_r = self.zip_dtypes()
        ent = np.ascontiguousarray(entries, dtype=dt_e)
        res = np.zeros(len(ent), dtype=dt_r)
        alen = ctypes.c_uint64(0)
        rc = self.lib.zada_zip_device(self.ctx, method, len(ent), ent.ctypes.data if len(ent) else None, d_archive_ptr, cap, archive_base, ctypes.byref(alen),
                                      res.ctypes.data if len(ent) else None)
        if rc != 0:
            self._err(rc, "zada_zip_device")
        return alen.value, res

    def zip_bound_ex(self, entries, archive_base=0, encrypted=False):
        """zada_zip_bound_ex: the bound for zip_device_ex (encrypted: 12 bytes of encryption header more per entry)."""
        import numpy as np
        ent = np.ascontiguousarray(entries, dtype=self.zip_dtypes()[0])
        return int(self.lib.zada_zip_bound_ex(len(ent), ent.ctypes.data if len(ent) else None, archive_base, 1 if encrypted else 0))

    def zip_device_ex(self, entries, d_archive_ptr, cap, method, archive_base=0, password=None, headers=None, legacy=False):
        """zada_zip_device_ex: zip_device with every method Zip.Create takes -- Shrink_1 and Reduce_1 .. _4 only with legacy=True, which sets the knob
        "zip_legacy" around the call --, and with a password (bytes, or str taken as Latin-1).
        headers: eleven bytes per entry for the encryption headers -- one bytes object, or a list of them --, os.urandom by default.  An LZMA_3* entry
        the coder refuses raises ReferenceDefect."""
        import numpy as np
        dt_e, dt_r = self.zip_dtypes()
        ent = np.ascontiguousarray(entries, dtype=dt_e)
        res = np.zeros(len(ent), dtype=dt_r)
        alen = ctypes.c_uint64(0)
        crypt = None
        if password is not None:
            pw = _password(password)
            if headers is None:
                headers = os.urandom(11 * len(ent))
            elif not isinstance(headers, (bytes, bytearray)):
                headers = b"".join(bytes(h) for h in headers)
            if len(headers) != 11 * len(ent):
                raise ValueError("zip_device_ex: %d header bytes for %d entries" % (len(headers), len(ent)))
            keep = (ctypes.create_string_buffer(pw, len(pw)), ctypes.create_string_buffer(bytes(headers), max(len(headers), 1)))
            crypt = (ctypes.c_uint64 * 3)(ctypes.addressof(keep[0]), len(pw), ctypes.addressof(keep[1]))
        if legacy:
            self.set_knob("zip_legacy", 1)
        try:
            rc = self.lib.zada_zip_device_ex(self.ctx, method, len(ent), ent.ctypes.data if len(ent) else None, d_archive_ptr, cap, archive_base,
                                             ctypes.addressof(crypt) if crypt is not None else None, ctypes.byref(alen), res.ctypes.data if len(ent) else None)
        finally:
            if legacy:
                self.set_knob("zip_legacy", 0)
        if rc != 0:
            self._err(rc, "zada_zip_device_ex")
        return alen.value, res

    # ---- ReZip on device memory (include/zada.h "an archive in device memory recompressed into device memory") ----
    @staticmethod
    def rezip_dtypes():
        """(dtype of zada_rezip_entry, dtype of zada_rezip_result) as numpy structured types."""
        import numpy as np
        return (np.dtype([("in_off", "<u8"), ("n_in", "<u8"), ("usize", "<u8"), ("crc", "<u4"), ("time", "<u4"), ("method", "<u2"), ("flags", "<u2"), ("version", "<u2"),
                          ("pad", "<u2"), ("name_len", "<u4"), ("pad2", "<u4"), ("name", "<u8")]),
                np.dtype([("rc", "<i4"), ("approach", "<i4"), ("zip_type", "<u2"), ("flags", "<u2"), ("crc", "<u4"), ("csize", "<u8"), ("offset", "<u8")]))

    def rezip_bound(self, entries, comment_len=0):
        """zada_rezip_bound: an upper bound on the archive rezip_device makes of `entries`."""
        import numpy as np
        ent = np.ascontiguousarray(entries, dtype=self.rezip_dtypes()[0])
        return int(self.lib.zada_rezip_bound(len(ent), ent.ctypes.data if len(ent) else None, comment_len))

    def rezip_device(self, d_src_ptr, src_len, entries, d_archive_ptr, cap, approaches=RZ_DEFAULT, formats=RZ_ALL_FORMATS, archive_base=0, comment=b""):
        """zada_rezip_device: `entries` is a numpy structured array of rezip_dtypes () [0] rows (name: HOST addresses the caller keeps alive).  Returns
        (the archive's length, the structured array of results, the count x 12 matrix of sizes by approach, all ones where not tried)."""
        import numpy as np
        dt_e, dt_r = self.rezip_dtypes()
        ent = np.ascontiguousarray(entries, dtype=dt_e)
        res = np.zeros(len(ent), dtype=dt_r)
        sizes = np.zeros((len(ent), 12), dtype=np.uint64)
        alen = ctypes.c_uint64(0)
        keep = ctypes.create_string_buffer(bytes(comment), max(len(comment), 1))
        rc = self.lib.zada_rezip_device(self.ctx, d_src_ptr, src_len, len(ent), ent.ctypes.data if len(ent) else None, approaches, formats, d_archive_ptr, cap, archive_base,
                                        ctypes.addressof(keep) if comment else None, len(comment), ctypes.byref(alen), res.ctypes.data if len(ent) else None,
                                        sizes.ctypes.data if len(ent) else None)
        if rc != 0:
            self._err(rc, "zada_rezip_device")
        return alen.value, res, sizes

    # ---- Comp_Zip on device memory (include/zada.h "two archives that lie in device memory, compared entry by entry") ----
    def compare_device(self, d_a_ptr, d_b_ptr, n):
        """zada_compare_device: the first offset at which the n bytes at the two device addresses (any alignment) differ, or n."""
        first = ctypes.c_uint64(0)
        rc = self.lib.zada_compare_device(self.ctx, d_a_ptr, d_b_ptr, n, ctypes.byref(first))
        if rc != 0:
            self._err(rc, "zada_compare_device")
        return first.value

    @staticmethod
    def compzip_dtype():
        """dtype of zada_compzip_result as a numpy structured type."""
        import numpy as np
        return np.dtype([("verdict", "<i4"), ("rc_a", "<i4"), ("rc_b", "<i4"), ("crc_a", "<u4"), ("crc_b", "<u4"), ("pad", "<u4"), ("len_a", "<u8"), ("len_b", "<u8"),
                         ("position", "<u8"), ("compared", "<u8")])

    def compzip_device(self, d_a_ptr, len_a, d_b_ptr, len_b, rows_a, rows_b, keys0=None):
        """zada_compzip_device: rows_a / rows_b are numpy structured arrays of unzip_dtypes () [0] rows, pair by pair (CZ_ABSENT in a row of rows_b's
        flags: archive 2 has no such entry); keys0 the keys of the password or None.  Returns the structured array of results (compzip_dtype ()).
        An argument the call refuses raises ZadaError."""
        import numpy as np
        dt_e = self.unzip_dtypes()[0]
        ra, rb = np.ascontiguousarray(rows_a, dtype=dt_e), np.ascontiguousarray(rows_b, dtype=dt_e)
        if len(ra) != len(rb):
            raise ValueError("compzip_device: %d rows of archive 1, %d of archive 2" % (len(ra), len(rb)))
        res = np.zeros(len(ra), dtype=self.compzip_dtype())
        k = (ctypes.c_uint32 * 3)(*keys0) if keys0 is not None else None
        rc = self.lib.zada_compzip_device(self.ctx, d_a_ptr, len_a, d_b_ptr, len_b, len(ra), ra.ctypes.data if len(ra) else None, rb.ctypes.data if len(ra) else None, k,
                                          res.ctypes.data if len(ra) else None)
        if rc != 0:
            self._err(rc, "zada_compzip_device")
        return res

    # ---- Find_Zip on device memory (include/zada.h "a string searched in every entry of an archive that lies in device memory") ----
    def find_device(self, d_ptr, n, text, ignore_case=True):
        """zada_find_device: the n bytes at the device address (any alignment) as one entry, text the search string (bytes, or str taken as Latin-1).
        Returns (occurrences, first): what find_zip counts, and the offset of the last byte of the first occurrence, or n."""
        text = _search_text(text, check=False)
        occ, first = ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = self.lib.zada_find_device(self.ctx, d_ptr, n, text, len(text), FZ_IGNORE_CASE if ignore_case else 0, ctypes.byref(occ), ctypes.byref(first))
        if rc != 0:
            self._err(rc, "zada_find_device")
        return occ.value, first.value

    @staticmethod
    def findzip_dtype():
        """dtype of zada_findzip_result as a numpy structured type."""
        import numpy as np
        return np.dtype([("rc", "<i4"), ("crc", "<u4"), ("out_len", "<u8"), ("occurrences", "<u8"), ("first", "<u8")])

    def findzip_device(self, d_archive_ptr, archive_len, entries, text, ignore_case=True, keys0=None):
        """zada_findzip_device: `entries` is a numpy structured array of unzip_dtypes () [0] rows in the order they are to be searched, keys0 the keys of
        the password or None.  Returns the structured array of results (findzip_dtype ()).  An argument the call refuses raises ZadaError."""
        import numpy as np
        text = _search_text(text, check=False)
        ent = np.ascontiguousarray(entries, dtype=self.unzip_dtypes()[0])
        res = np.zeros(len(ent), dtype=self.findzip_dtype())
        k = (ctypes.c_uint32 * 3)(*keys0) if keys0 is not None else None
        rc = self.lib.zada_findzip_device(self.ctx, d_archive_ptr, archive_len, len(ent), ent.ctypes.data if len(ent) else None, k, text, len(text),
                                          FZ_IGNORE_CASE if ignore_case else 0, res.ctypes.data if len(ent) else None)
        if rc != 0:
            self._err(rc, "zada_findzip_device")
        return res

    def lz77_tokens(self, data, method=Method.Deflate_3):
        import numpy as np
        n = len(data)
        tok = np.zeros(n + 8, dtype=np.uint32)
        nt = ctypes.c_uint64(0)
        rc = self.lib.zada_lz77_tokens(self.ctx, method, _addr(data) if n else None, n, tok.ctypes.data, n + 8, ctypes.byref(nt))
        if rc != 0:
            self._err(rc, "zada_lz77_tokens")
        return tok[:nt.value]

    # ---- one stream over several contexts (include/zada.h "One stream over several contexts"; driver: sharding.py) ----
    def range_open(self, d_in_ptr, stream_size, lo, n, pre, post, method=Method.Deflate_3):
        rc = self.lib.zada_range_open(self.ctx, method, d_in_ptr, stream_size, lo, n, pre, post)
        if rc != 0:
            self._err(rc, "zada_range_open")

    def range_lz(self, entry=None):
        """entry: (pos, kind) the range before ended in, or None.  Returns dict(atoms, exit, warm, crc_raw, entry_known)."""
        info = _RangeInfo()
        e = _ParseState(entry[0], entry[1], 0) if entry is not None else None
        rc = self.lib.zada_range_lz(self.ctx, ctypes.addressof(e) if e is not None else None, ctypes.addressof(info))
        if rc != 0:
            self._err(rc, "zada_range_lz")
        return dict(atoms=info.atoms, exit=(info.exit.pos, info.exit.kind), warm=(info.warm.pos, info.warm.kind),
                    crc_raw=info.crc_raw, entry_known=bool(info.entry_known))

    def range_edges(self, head_atoms_ptr, head_pos_ptr, tail_atoms_ptr, tail_pos_ptr):
        nh, nt = ctypes.c_uint32(0), ctypes.c_uint32(0)
        rc = self.lib.zada_range_edges(self.ctx, head_atoms_ptr, head_pos_ptr, ctypes.byref(nh), tail_atoms_ptr, tail_pos_ptr, ctypes.byref(nt))
        if rc != 0:
            self._err(rc, "zada_range_edges")
        return nh.value, nt.value

    def range_place(self, atoms_before, atoms_total, lb_atoms_ptr=None, lb_pos_ptr=None, n_lb=0, la_atoms_ptr=None, la_pos_ptr=None, n_la=0):
        rc = self.lib.zada_range_place(self.ctx, atoms_before, atoms_total, lb_atoms_ptr, lb_pos_ptr, n_lb, la_atoms_ptr, la_pos_ptr, n_la)
        if rc != 0:
            self._err(rc, "zada_range_place")

    def range_analyze(self):
        rc = self.lib.zada_range_analyze(self.ctx)
        if rc != 0:
            self._err(rc, "zada_range_analyze")

    def range_choose(self, carry_in=None):
        """carry_in: the 352-byte state of the range before (None: the stream starts here).
        Returns (carry_out bytes, bit_begin, bit_end)."""
        cin = ctypes.create_string_buffer(bytes(carry_in), CARRY_BYTES) if carry_in is not None else None
        cout = ctypes.create_string_buffer(CARRY_BYTES)
        b0, b1 = ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = self.lib.zada_range_choose(self.ctx, ctypes.addressof(cin) if cin is not None else None, ctypes.addressof(cout),
                                        ctypes.byref(b0), ctypes.byref(b1))
        if rc != 0:
            self._err(rc, "zada_range_choose")
        return cout.raw, b0.value, b1.value

    def range_emit(self, d_out_ptr, cap):
        nb = ctypes.c_uint64(0)
        rc = self.lib.zada_range_emit(self.ctx, d_out_ptr, cap, ctypes.byref(nb))
        if rc != 0:
            self._err(rc, "zada_range_emit")
        return nb.value

    def crc32_combine(self, reg, raw, length):
        return self.lib.zada_crc32_combine(reg, raw, length)

    def last_blocks(self):
        import numpy as np
        nb = ctypes.c_uint64(0)
        self.lib.zada_last_blocks(self.ctx, None, 0, ctypes.byref(nb))
        rec = np.zeros((max(nb.value, 1), 4), dtype=np.uint64)
        self.lib.zada_last_blocks(self.ctx, rec.ctypes.data, nb.value, ctypes.byref(nb))
        return rec[:nb.value]

    def last_trace(self):
        """Similarity tests of the block splitter in the last call: array of (atom, L1 distance, cut level or 0)."""
        import numpy as np
        k = ctypes.c_uint64(0)
        self.lib.zada_last_trace(self.ctx, None, 0, ctypes.byref(k))
        rec = np.zeros((max(k.value, 1), 3), dtype=np.uint64)
        self.lib.zada_last_trace(self.ctx, rec.ctypes.data, k.value, ctypes.byref(k))
        return rec[:k.value]

    def last_timing(self):
        names = (ctypes.c_char_p * 64)()
        ms = (ctypes.c_float * 64)()
        k = self.lib.zada_last_timing(self.ctx, ctypes.cast(names, ctypes.c_void_p), ctypes.cast(ms, ctypes.c_void_p), 64)
        return [(names[i].decode(), ms[i]) for i in range(k)]


def silesia_mix(nbytes, seed=0x5A1E51A, class_mask=0x1F, offset=0, version=1):
    """Deterministic synthetic corpus (csrc/silesia_mix.c), as a numpy uint8 array.  version 1 = "silesia_mix_v1" (what the committed
    golden digests were taken on; its 64 KiB segments are shifted copies of one stream of draws, which only encoders that look
    further back than 32 KiB can see), version 2 = "silesia_mix_v2" (segments seeded independently: the benchmark stream)."""
    import numpy as np
    L = load_library()
    b = np.zeros(nbytes, dtype=np.uint8)
    if nbytes:
        (L.zada_silesia_mix_v2 if version >= 2 else L.zada_silesia_mix)(seed, class_mask, offset, nbytes, b.ctypes.data)
    return b


class ZipCreate:
    """Zip.Create on a memory stream: Create_Archive / Add_Stream / Finish
    (zip_lib/zip-create.adb:36-58, 194-297, 645-756; headers zip-headers.adb:168-195, 244-276, 494-511), incl. the
    promotion to Zip_64 (Check_Size zip-create.adb:161-179; local header extension :237-251, 283-289 and
    zip-headers.adb:197-210, 336-355; central extension and Zip64 end records zip-create.adb:682-752,
    zip-headers.adb:534-579)."""

    DEFAULT_TIME = 16789 * 65536  # zip_streams.ads:223
    _MARGIN = 22 + 56 + 20 + 2 ** 16 + 10   # Check_Size, zip-create.adb:165-169

    def __init__(self, encoder, method=Method.Deflate_3, _offset_bias=0):
        self.enc, self.method = encoder, method
        self.buf = bytearray()
        self.entries = []
        self.zip64 = False
        self._bias = _offset_bias       # test hook: pretend that this many bytes precede the buffer

    def _check_size(self, value):
        if not self.zip64 and value >= 2 ** 32 - self._MARGIN:
            self.zip64 = True

    @staticmethod
    def _needs_zip64(csize, usize, offset):      # Needs_Local_Zip_64_Header_Extension, zip-headers.adb:197-210
        return csize >= 0xFFFFFFFF or usize >= 0xFFFFFFFF or offset >= 0xFFFFFFFF

    def _presel(self):
        return self.method in (Method.Preselection_1, Method.Preselection_2)

    def add_stream(self, name, data, file_time=None, unicode_name=True, password=None, _header=None):
        """Add_Stream (zip-create.adb:194-297).  password (bytes, or str taken as Latin-1): the entry is encrypted (Compress_Data's password,
        :253-265); _header is a test hook: the eleven random bytes of the encryption header."""
        # (Preselection: the content hint is Guess_Type_from_Name of the entry's name, zip-create.adb:261)
        hint = guess_type_from_name(name) if self._presel() else None
        if password is None:
            payload, crc, zt = self.enc.compress_data(data, self.method, content_hint=hint)
            return self.add_compressed(name, payload, crc, len(data), zt, file_time, unicode_name)
        payload, crc, zt = self.enc.compress_data(data, self.method, content_hint=hint, password=password, header=_header)
        return self.add_compressed(name, payload, crc, len(data), zt, file_time, unicode_name, password=password)

    def _batch(self, datas, method):
        if method == Method.Store:
            return [(1, None, 0)] * len(datas)
        if Method.BZip2_1 <= method <= Method.BZip2_3:
            return self.enc.bzip2_batch(datas, method)
        if Method.LZMA_0 <= method <= Method.LZMA_for_AU:
            return self.enc.lzma_batch(datas, method)
        if method == Method.Shrink_1:
            return self.enc.shrink_batch(datas)
        if Method.Reduce_1 <= method <= Method.Reduce_4:
            return self.enc.reduce_batch(datas, method)
        return self.enc.deflate_batch(datas, method)

    def add_streams(self, names, datas, file_time=None, unicode_name=True, password=None, _headers=None):
        """Add_Stream for many entries at once: the entries are compressed as one batch (zada_deflate_batch: one launch
        sequence for all the small ones), with Compress_Data's Store fallback (zip-compress.adb:224-237) and CRC Init / Final
        (:144, 218) per entry.  The archive is the one Add_Stream after Add_Stream writes.  Preselection: every entry's method is
        preselect (method, Guess_Type_from_Name (name), size); the entries of one method go through its batch entry point together.
        With a password the entries are compressed the same way; their encryption headers are made on the host (twelve serial bytes each) and all
        payloads -- those that fell back to Store too -- are encoded by one crypt_encode_batch.  _headers (test hook): eleven bytes per entry."""
        import zlib
        names, datas = list(names), list(datas)
        if password is not None:
            _password(password)
        if self._presel():
            methods = [preselect(self.method, guess_type_from_name(nm), len(d)) for nm, d in zip(names, datas)]
        else:
            methods = [self.method] * len(datas)
        res = [None] * len(datas)
        for m in sorted(set(methods)):
            idx = [i for i, mi in enumerate(methods) if mi == m]
            for i, r in zip(idx, self._batch([datas[i] for i in idx], m)):
                res[i] = r
        plain = []                                   # (name, payload, final CRC-32, size, zip_type) as an unencrypted archive takes them
        for name, data, m, (rc, payload, crc) in zip(names, datas, methods, res):
            if rc == 0:
                plain.append((name, payload, crc ^ 0xFFFFFFFF, len(data), _zip_type(m)))
            else:
                plain.append((name, bytes(data), (zlib.crc32(data) if m == Method.Store else crc ^ 0xFFFFFFFF) & 0xFFFFFFFF, len(data), 0))
        if password is not None:
            k0 = self.enc.crypt_init_keys(password)
            hdrs, keys = [], []
            for i, (_, _, crc, _, _) in enumerate(plain):
                h, k = self.enc.crypt_header(k0, os.urandom(11) if _headers is None else _headers[i], crc)
                hdrs.append(h); keys.append(k)
            coded = self.enc.crypt_encode_batch(keys, [p[1] for p in plain])
            for (name, _, crc, usize, zt), h, (ct, _) in zip(plain, hdrs, coded):
                self.add_compressed(name, h + ct, crc, usize, zt, file_time, unicode_name, password=password)
            return
        for name, payload, crc, usize, zt in plain:
            self.add_compressed(name, payload, crc, usize, zt, file_time, unicode_name)

    def add_compressed(self, name, payload, crc, usize, zt, file_time=None, unicode_name=True, password=None, flag_bits=0):
        """Entry whose payload was compressed elsewhere (another rank / GPU): the bytes written
        are those Add_Stream would have written for the same payload.  With a password the payload is what Compress_Data left for it -- the
        encryption header and the encoded stream -- and the entry carries Encryption_Flag_Bit (zip-create.adb:221-223).  flag_bits: an Implode
        payload's (zt = 6) general-purpose bits 1 and 2 -- 8 KiB dictionary, three trees --, which say how it was written; ignored otherwise."""
        nm = name.replace("\\", "/").encode("utf-8")
        e = dict(name=nm, flag=(0x0800 if unicode_name else 0) | (0x0002 if zt == 14 else 0) | (0x0001 if password else 0) | (flag_bits & 6 if zt == 6 else 0),   # LZMA_EOS_Flag_Bit, zip-create.adb:266-278
                 zip_type=zt, time=self.DEFAULT_TIME if file_time is None else file_time,
                 crc=crc, csize=len(payload), usize=usize, offset=len(self.buf) + self._bias)
        self._check_size(usize)
        # the local header's form is decided before compression, on the provisional sizes (:231-241)
        z64 = self._needs_zip64(usize, usize, e["offset"])
        if z64:
            hdr = struct.pack("<4sHHHIIIIHH", b"PK\x03\x04", 10, e["flag"], zt, e["time"], crc, 0xFFFFFFFF, 0xFFFFFFFF, len(nm), 20)
            ext = struct.pack("<HHQQ", 1, 16, usize, e["csize"])
        else:
            hdr = struct.pack("<4sHHHIIIIHH", b"PK\x03\x04", 10, e["flag"], zt, e["time"], crc, e["csize"], usize, len(nm), 0)
            ext = b""
        self.buf += hdr + nm + ext + payload
        self.entries.append(e)
        return e["csize"], zt

    def write_device(self, names, tensors, file_time=None, unicode_name=True):
        """add_streams + finish for entries that lie in device memory: tensors are contiguous torch.uint8 tensors on the encoder's device (empty ones
        are allowed).  ONE zada_zip_device call writes the complete archive -- the bytes add_streams and finish write for the same inputs -- into a
        tensor on that device; no entry byte crosses the host.  Returns the archive as a view of that tensor; self.entries is what add_compressed
        would have recorded (self.buf stays empty).  Only on a ZipCreate that has no entries yet, with method Store or a Deflate method.
        The view keeps the whole allocation of zada_zip_bound bytes alive -- the inputs' size plus the headers, however small the archive turns out:
        .clone() it to let the rest go.  A name longer than 65 535 bytes is refused by the C call (ZadaError with the entry's index), where
        add_compressed fails in struct.pack."""
        import torch
        tab, nms, _blob, dev = self._device_table(names, tensors, file_time, unicode_name, "ZipCreate.write_device")
        cap = self.enc.zip_bound(tab, self._bias)
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        alen, res = self.enc.zip_device(tab, out.data_ptr(), cap, self.method, self._bias)
        self._device_entries(tab, nms, res, 0x0800 if unicode_name else 0)
        return out[:alen]

    def _device_table(self, names, tensors, file_time, unicode_name, who):
        """The table of zada_zip_entry rows of write_device / write_device_ex (and the names' bytes it points into, which the caller keeps alive)."""
        import numpy as np
        import torch
        if self.entries or self.buf:
            raise ValueError("%s: the archive already has entries" % who)
        names, tensors = list(names), list(tensors)
        if len(names) != len(tensors):
            raise ValueError("%s: %d names for %d tensors" % (who, len(names), len(tensors)))
        dev = torch.device("cuda", self.enc.device)
        for t in tensors:
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_contiguous() or (t.numel() and t.device != dev):
                raise ZadaError("%s: contiguous torch.uint8 tensors on %s are needed" % (who, dev))
        nms = [nm.replace("\\", "/").encode("utf-8") for nm in names]
        n = len(nms)
        tab = np.zeros(n, dtype=self.enc.zip_dtypes()[0])
        blob = np.frombuffer(b"".join(nms) + b"\0", dtype=np.uint8)          # the names one behind the other: the table points into it
        nlen = np.fromiter((len(nm) for nm in nms), np.uint64, n)
        tab["name"] = np.uint64(blob.ctypes.data) + np.cumsum(nlen) - nlen
        tab["name_len"] = np.minimum(nlen, 0xFFFFFFFF)
        tab["n"] = np.fromiter((t.numel() for t in tensors), np.uint64, n)
        tab["d_data"] = np.fromiter((t.data_ptr() if t.numel() else 0 for t in tensors), np.uint64, n)
        tab["time"] = self.DEFAULT_TIME if file_time is None else file_time
        tab["flags"] = 1 if unicode_name else 0
        return tab, nms, blob, dev

    def _device_entries(self, tab, nms, res, flag):
        for k, nm in enumerate(nms):
            r = res[k]
            usize = int(tab["n"][k])
            zt = int(r["zip_type"])
            self._check_size(usize)
            self.entries.append(dict(name=nm, flag=flag | (0x0002 if zt == 14 else 0), zip_type=zt, time=int(tab["time"][k]),
                                     crc=int(r["crc"]), csize=int(r["csize"]), usize=usize, offset=int(r["offset"])))

    def write_device_ex(self, names, tensors, file_time=None, unicode_name=True, password=None, _headers=None, legacy=False):
        """write_device through zada_zip_device_ex: any method of this ZipCreate -- BZip2, LZMA, Preselection_1 / _2 by the entries' names and sizes;
        Shrink_1 and Reduce_1 .. _4 only with legacy=True (one wave per entry: a batch of small entries fills the device, one large entry is slow) --
        and, with a password (bytes, or str taken as Latin-1), encrypted entries; _headers (test hook): eleven bytes per
        entry.  The archive is the one add_streams + finish write for the same inputs; self.entries is what add_compressed would have recorded,
        flag bits included.  write_device's rules hold: contiguous torch.uint8 tensors on the encoder's device, empty ones allowed, only on a
        ZipCreate without entries.  Returns the archive as a view of a tensor of zada_zip_bound_ex bytes."""
        import torch
        pw = None if password is None else _password(password)
        tab, nms, _blob, dev = self._device_table(names, tensors, file_time, unicode_name, "ZipCreate.write_device_ex")
        cap = self.enc.zip_bound_ex(tab, self._bias, pw is not None)
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        alen, res = self.enc.zip_device_ex(tab, out.data_ptr(), cap, self.method, self._bias, password=pw, headers=_headers, legacy=legacy)
        self._device_entries(tab, nms, res, (0x0800 if unicode_name else 0) | (0x0001 if pw else 0))
        return out[:alen]

    def finish(self):
        cd_off = len(self.buf) + self._bias
        if not self.zip64 and len(self.entries) >= 0xFFFF:
            self.zip64 = True
        cd_size = 0
        for e in self.entries:
            z64 = self._needs_zip64(e["csize"], e["usize"], e["offset"])
            if z64:
                self.zip64 = True
            m = 0xFFFFFFFF
            self.buf += struct.pack("<4sHHHHIIIIHHHHHII", b"PK\x01\x02", 23, 10, e["flag"], e["zip_type"], e["time"], e["crc"],
                                    m if z64 else e["csize"], m if z64 else e["usize"], len(e["name"]), 28 if z64 else 0, 0, 0, 0, 0,
                                    m if z64 else e["offset"]) + e["name"]
            if z64:
                self.buf += struct.pack("<HHQQQ", 1, 24, e["usize"], e["csize"], e["offset"])
            cd_size += 46 + len(e["name"]) + (28 if z64 else 0)
        if self.entries:
            self._check_size(len(self.buf) + self._bias + 1)
        n = len(self.entries)
        if self.zip64:
            e64_off = len(self.buf) + self._bias
            self.buf += struct.pack("<4sQHHIIQQQQ", b"PK\x06\x06", 44, 0x2D, 0x2D, 0, 0, n, n, cd_size, cd_off)
            self.buf += struct.pack("<4sIQI", b"PK\x06\x07", 0, e64_off, 1)
            self.buf += struct.pack("<4sHHHHIIH", b"PK\x05\x06", 0, 0, 0xFFFF, 0xFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0)
        else:
            self.buf += struct.pack("<4sHHHHIIH", b"PK\x05\x06", 0, 0, n, n, cd_size, cd_off, 0)
        return bytes(self.buf)


class ZipEntry:
    """One entry of an archive's central directory (Zip.Zip_Info's Dir_node)."""
    __slots__ = ("name", "raw_name", "method", "flags", "crc", "csize", "usize", "header_offset", "data_offset", "dos_time", "encrypted",
                 "local_version", "local_flags", "local_time")      # the local header's version needed, bit flag and DOS time (what ReZip keeps)

    def __repr__(self):
        return "ZipEntry(%r, method=%d, csize=%d, usize=%d)" % (self.name, self.method, self.csize, self.usize)


class ZipInfo:
    """Zip.Load (zip_lib/zip.adb, zip-headers.adb): the central directory of an archive held in memory.  Pure Python, needs no GPU.
    .entries: ZipEntry (name, method code, flags, CRC, sizes, header and data offset), in directory order; .comment: the archive comment.
    Sizes and CRC are the central directory's, so entries written with a data descriptor (flag bit 3) need no second look.  An archive
    with bytes in front of it (offsets that do not start at the buffer) is read with the shift the end record implies.
    load (bytes) keeps the archive in .data; load_device (tensor) keeps the tensor in .device_data (.data is None) and reads only the directory."""

    def __init__(self, data, entries, comment, device_data=None):
        self.data, self.entries, self.comment, self.device_data = data, entries, comment, device_data

    def __getitem__(self, name):
        for e in self.entries:
            if e.name == name:
                return e
        raise KeyError(name)

    @classmethod
    def load(cls, archive_bytes):
        data = bytes(archive_bytes)
        entries, comment = cls._parse(len(data), lambda lo, hi: data[lo:hi], lambda offs: [data[h:h + 30] for h in offs])
        return cls(data, entries, comment)

    @classmethod
    def load_device(cls, tensor):
        """The same entries, comment and errors as load (bytes (tensor)) for an archive held in a contiguous one-dimensional torch.uint8 tensor, on cpu or
        cuda, without copying it: only the last 22 + 65 535 bytes, the Zip64 records, the central directory and -- in one gather and one copy -- the
        30-byte local headers of the entries are fetched (a Zip64 end record that is not where the locator implies is searched for in everything before
        it, as load does).  For UnZip.extract_device."""
        import torch
        if not isinstance(tensor, torch.Tensor) or tensor.dtype != torch.uint8 or tensor.dim() != 1 or not tensor.is_contiguous():
            raise ZadaError("ZipInfo.load_device: a contiguous one-dimensional torch.uint8 tensor is needed")
        n = tensor.numel()

        def fetch(lo, hi):
            lo, hi = max(lo, 0), min(hi, n)
            return tensor[lo:hi].cpu().numpy().tobytes() if hi > lo else b""

        def fetch_locals(offs):
            if not offs:
                return []
            at = torch.tensor(offs, dtype=torch.int64, device=tensor.device)
            rows = tensor[at[:, None] + torch.arange(30, dtype=torch.int64, device=tensor.device)].cpu().numpy()
            return [rows[i].tobytes() for i in range(len(offs))]
        entries, comment = cls._parse(n, fetch, fetch_locals)
        return cls(None, entries, comment, tensor)

    @staticmethod
    def _parse(n, fetch, fetch_locals):
        """The directory of an archive of n bytes: fetch (lo, hi) gives its bytes [lo, hi) (0 <= lo), fetch_locals (offsets) the 30 bytes at every offset
        (each with offset + 30 <= n).  -> (entries, comment)"""
        try:
            # end-of-central-directory record: the last one whose comment ends where the archive ends (zip-headers.adb:412-492)
            lo = max(0, n - 22 - 65535)
            t = fetch(lo, n)
            rel = t.rfind(b"PK\x05\x06")
            while rel >= 0:
                if rel + 22 <= len(t) and rel + 22 + struct.unpack_from("<H", t, rel + 20)[0] == len(t):
                    break
                rel = t.rfind(b"PK\x05\x06", 0, rel)
            if rel < 0:
                raise ZadaError("ZipInfo.load: no end-of-central-directory record (not a Zip archive)")
            pos = lo + rel
            _, disk, cd_disk, n_here, total, cd_size, cd_off, clen = struct.unpack_from("<4sHHHHIIH", t, rel)
            comment = t[rel + 22:rel + 22 + clen]
            tail = pos                                     # where the central directory's records end
            if pos >= 20 and fetch(pos - 20, pos - 16) == b"PK\x06\x07":       # Zip64 locator, then the Zip64 end record (zip-headers.adb:534-579)
                p64 = pos - 20 - 56
                if p64 < 0 or fetch(p64, p64 + 4) != b"PK\x06\x06":
                    p64 = fetch(0, pos - 20).rfind(b"PK\x06\x06")
                if p64 < 0:
                    raise ZadaError("ZipInfo.load: Zip64 locator without a Zip64 end record")
                _, _, _, _, _, _, _, total, cd_size, cd_off = struct.unpack_from("<4sQHHIIQQQQ", fetch(p64, p64 + 56), 0)
                tail = p64
            cd_pos = tail - cd_size
            if cd_pos < 0 or cd_size > n:
                raise ZadaError("ZipInfo.load: the central directory lies beyond the file")
            shift = cd_pos - cd_off                        # bytes in front of the archive (negative: the archive was cut out of a larger file)
            data = fetch(cd_pos, tail)
            # the central headers; what is wrong with one is raised once the local headers of the entries before it have been looked at, in the
            # order of one pass over the archive
            entries, p, pending = [], 0, None
            for _ in range(total):
                if p + 46 > len(data) or data[p:p + 4] != b"PK\x01\x02":
                    pending = ZadaError("ZipInfo.load: truncated or damaged central header at %d" % (cd_pos + p))
                    break
                (_, _, _, flags, method, dos_time, crc, csize, usize, nlen, xlen, clen2, _, _, _, off) = struct.unpack_from("<4sHHHHIIIIHHHHHII", data, p)
                if p + 46 + nlen + xlen + clen2 > len(data):
                    pending = ZadaError("ZipInfo.load: truncated central header at %d" % (cd_pos + p))
                    break
                raw = data[p + 46:p + 46 + nlen]
                extra = data[p + 46 + nlen:p + 46 + nlen + xlen]
                q = 0
                while q + 4 <= len(extra):                 # the Zip64 extended information: only the fields that are 0xFFFFFFFF above, in this order
                    tag, sz = struct.unpack_from("<HH", extra, q)
                    if tag == 1:
                        f = q + 4
                        vals = []
                        while f + 8 <= q + 4 + sz and f + 8 <= len(extra):
                            vals.append(struct.unpack_from("<Q", extra, f)[0]); f += 8
                        if usize == 0xFFFFFFFF and vals:
                            usize = vals.pop(0)
                        if csize == 0xFFFFFFFF and vals:
                            csize = vals.pop(0)
                        if off == 0xFFFFFFFF and vals:
                            off = vals.pop(0)
                    q += 4 + sz
                e = ZipEntry()
                e.raw_name, e.name = raw, raw.decode("utf-8" if flags & 0x800 else "cp437", "replace")
                e.method, e.flags, e.crc, e.csize, e.usize, e.dos_time = method, flags, crc, csize, usize, dos_time
                e.encrypted = bool(flags & 1)
                e.header_offset = off + shift
                entries.append(e)
                p += 46 + nlen + xlen + clen2
            # the local headers: the thirty bytes in front of every entry's name
            rows = iter(fetch_locals([e.header_offset for e in entries if 0 <= e.header_offset <= n - 30]))
            for e in entries:
                h = e.header_offset
                row = next(rows) if 0 <= h <= n - 30 else b""
                if row[:4] != b"PK\x03\x04":
                    raise ZadaError("ZipInfo.load: entry %r: no local header at %d" % (e.name, h))
                lnl, lxl = struct.unpack_from("<HH", row, 26)
                e.local_version, e.local_flags, _, e.local_time = struct.unpack_from("<HHHI", row, 4)
                e.data_offset = h + 30 + lnl + lxl
                if e.data_offset + e.csize > n:
                    raise ZadaError("ZipInfo.load: entry %r: its data lie beyond the file" % e.name)
            if pending is not None:
                raise pending
            return entries, comment
        except (struct.error, IndexError) as ex:
            raise ZadaError("ZipInfo.load: damaged archive (%s)" % ex)


class UnZip:
    """UnZip.Extract (unzip.ads:55-290) on an archive in memory: Store (0), Deflate (8) and Deflate64 (9) entries; all Deflate entries of a call go
    through ONE inflate_batch (one wave per entry), encrypted ones first through one crypt_decode_batch; size and CRC-32 -- computed on the device --
    are compared with the directory.  BZip2, LZMA and the older formats are not decoded: UnsupportedMethod.
    UnZip (encoder, bzip2=True) also decodes BZip2 (12) entries: all of a call through ONE bunzip2_batch (their blocks in parallel), with the same
    checks and errors; the default leaves them UnsupportedMethod.  UnZip (encoder, lzma=True) likewise decodes LZMA (14) entries: all of a call
    through ONE unlzma_batch (one wave per entry), eos = bit 1 of the entry's flags, cap = its uncompressed size; an entry whose stream ended on a
    marker with fewer bytes than promised is a SizeError.  Without lzma=True, LZMA entries are UnsupportedMethod.
    extract_device does the same for an archive that lies in device memory (ZipInfo.load_device), into device memory, in ONE zada_unzip_device call.
    UnZip (encoder, parallel_inflate=KiB) -- experimental -- sends Deflate entries whose compressed size is at least that many KiB through
    Encoder.inflate_par, one stream on many waves: extract calls it entry by entry (last_parallel lists their records), extract_device sets the knob
    "inflate_par_min_kib" around its call (Encoder.inflate_par_last then holds the sums).  Results, exceptions and texts are the default's.
    With parallel_deflate64=True as well, Deflate64 entries of that size go the same way (the knob "inflate_par_deflate64", set around the calls
    and put back; 4 bytes of workspace per output byte where Deflate takes 2).
    With parallel_batch=True as well -- experimental too -- extract_device sets the knob "inflate_par_batch" around its call and puts it back: the
    entries parallel_inflate selects then share their launches instead of running one after the other, which is what an archive of many entries
    of some MiB wants (README, "Parallel Inflate, batched").  extract on host bytes ignores it: that path calls inflate_par entry by entry.
    UnZip (encoder, legacy=True) also decodes Shrink (1), Reduce (2 .. 5) and Implode (6) entries: all of a call through ONE unlegacy_batch (one wave
    per entry; an Implode entry's general-purpose bits 1 and 2 say how it was written); extract_device sets the knob "unzip_legacy" around its call.
    Without legacy=True they are UnsupportedMethod, in the words of before."""

    _NAMES = {1: "Shrink", 2: "Reduce_1", 3: "Reduce_2", 4: "Reduce_3", 5: "Reduce_4", 6: "Implode", 12: "BZip2", 14: "LZMA", 98: "PPMd", 99: "AES"}
    _STREAMS = {1: "Shrink", 2: "Reduce", 3: "Reduce", 4: "Reduce", 5: "Reduce", 6: "Implode", 8: "Deflate", 9: "Deflate64", 12: "BZip2", 14: "LZMA"}

    def __init__(self, encoder, bzip2=False, lzma=False, parallel_inflate=None, legacy=False, parallel_deflate64=False, parallel_batch=False):
        self.enc = encoder
        self.bzip2 = bool(bzip2)
        self.lzma = bool(lzma)
        self.legacy = bool(legacy)
        if parallel_inflate is not None and int(parallel_inflate) < 1:
            raise ZadaError("UnZip: parallel_inflate is a size in KiB, at least 1, or None")
        self.parallel_inflate = None if parallel_inflate is None else int(parallel_inflate)
        if parallel_deflate64 and self.parallel_inflate is None:
            raise ZadaError("UnZip: parallel_deflate64 needs parallel_inflate, the size in KiB from which an entry goes the parallel way")
        self.parallel_deflate64 = bool(parallel_deflate64)
        if parallel_batch and self.parallel_inflate is None:
            raise ZadaError("UnZip: parallel_batch needs parallel_inflate, the size in KiB from which an entry goes the parallel way")
        self.parallel_batch = bool(parallel_batch)
        self.last_parallel = []                            # extract: (name, inflate_par_last ()) of the entries that went through inflate_par

    def _unsupported(self, e):
        """The UnsupportedMethod of an entry this reader's gates exclude, or None."""
        if e.method in (0, 8, 9) or (self.bzip2 and e.method == 12) or (self.lzma and e.method == 14) or (self.legacy and 1 <= e.method <= 6):
            return None
        if self.lzma:
            return UnsupportedMethod("entry %r: method %d (%s) is not decoded by this reader: Store, Deflate, Deflate64%s and LZMA only%s"
                                     % (e.name, e.method, self._NAMES.get(e.method, "unknown"), ", BZip2" if self.bzip2 else "",
                                        "" if self.bzip2 else " -- BZip2 decoding is out of scope"))
        if self.bzip2:
            return UnsupportedMethod("entry %r: method %d (%s) is not decoded by this reader: Store, Deflate, Deflate64 and BZip2 only -- LZMA decoding is out of scope"
                                     % (e.name, e.method, self._NAMES.get(e.method, "unknown")))
        return UnsupportedMethod("entry %r: method %d (%s) is not decoded by this reader: Store, Deflate and Deflate64 only -- BZip2 and LZMA decoding are out of scope"
                                 % (e.name, e.method, self._NAMES.get(e.method, "unknown")))

    @classmethod
    def _verdict(cls, e, rc, ol, reg):
        """What a decoder's (rc, bytes written, CRC register) -- a stored entry's (0, bytes stored, register) -- mean against the directory: None, or
        the DataError, SizeError or CRCError of the entry."""
        if rc != 0:
            return DataError("entry %r: not a valid %s stream, or longer than the %d bytes promised" % (e.name, cls._STREAMS.get(e.method, "Store"), e.usize))
        if ol != e.usize:
            return SizeError("entry %r: %d bytes %s, %d promised" % (e.name, ol, "stored" if e.method == 0 else "decoded", e.usize))
        if reg ^ 0xFFFFFFFF != e.crc:
            return CRCError("entry %r: CRC-32 %08x, the directory says %08x" % (e.name, reg ^ 0xFFFFFFFF, e.crc))
        return None

    @staticmethod
    def _finish(ents, res, test_only, errors):
        out = {e.name: res[k] for k, e in enumerate(ents)}
        if test_only or errors == "collect":
            return out
        for v in out.values():
            if isinstance(v, Exception):
                v.results = out
                raise v
        return out

    def extract(self, info, what=None, password=None, test_only=False, errors="raise"):
        """info: ZipInfo; what: None = every entry, or names.  Returns {name: bytes}.  An entry that fails is a WrongPassword, DataError, SizeError,
        CRCError or UnsupportedMethod: with errors = "raise" (default) the first of them is raised once every other entry has been extracted, the
        whole result in its .results; with errors = "collect" the exception stands in the result in place of the bytes.
        test_only = True: {name: None or the exception} -- the per-entry verdicts, no bytes; the decoded bytes never leave the device."""
        import zlib
        ents = info.entries if what is None else [info[nm] for nm in ([what] if isinstance(what, str) else what)]
        res, payload = {}, {}
        enc_idx = []
        for k, e in enumerate(ents):
            ex = self._unsupported(e)
            if ex is not None:
                res[k] = ex
                continue
            payload[k] = info.data[e.data_offset:e.data_offset + e.csize]
            if e.encrypted:
                if password is None:
                    res[k] = WrongPassword("entry %r is encrypted and no password was given" % e.name)
                elif e.csize < 12:
                    res[k] = DataError("entry %r: shorter than its encryption header" % e.name)
                else:
                    enc_idx.append(k)
        if enc_idx:
            k0 = self.enc.crypt_init_keys(password)
            for k, (plain, _) in zip(enc_idx, self.enc.crypt_decode_batch([k0] * len(enc_idx), [payload[k] for k in enc_idx])):
                e = ents[k]
                check = (e.dos_time >> 8) & 0xFF if e.flags & 8 else e.crc >> 24            # the header's last byte (zip-compress.adb:153-161; bit 3: the time stamp)
                if plain[11] != check:
                    res[k] = WrongPassword("entry %r: wrong password" % e.name)
                else:
                    payload[k] = plain[12:]

        def settle(todo, got):
            for k, (rc, out, ol, _, reg) in zip(todo, got):
                ex = self._verdict(ents[k], rc, ol, reg)
                res[k] = ex if ex is not None else None if test_only else out
        self.last_parallel = []
        if self.parallel_inflate is not None:
            was = self._deflate64_knob()
            try:
                for k, e in enumerate(ents):
                    if k in res or e.method not in ((8, 9) if self.parallel_deflate64 else (8,)) or len(payload[k]) < self.parallel_inflate << 10:
                        continue
                    try:
                        out, used, reg = self.enc.inflate_par(payload[k], e.usize, format=e.method)
                        settle([k], [(0, out, len(out), used, reg)])
                    except DataError:
                        settle([k], [(E_DATA, None, 0, 0, 0)])
                    self.last_parallel.append((e.name, self.enc.inflate_par_last()))
            finally:
                self._deflate64_knob(was)
        todo = [k for k in range(len(ents)) if k not in res and ents[k].method in (8, 9)]
        if todo:
            settle(todo, self.enc.inflate_batch([payload[k] for k in todo], [ents[k].usize for k in todo], [ents[k].method for k in todo], deliver=not test_only))
        todo = [k for k in range(len(ents)) if k not in res and ents[k].method == 12]
        if todo:
            settle(todo, self.enc.bunzip2_batch([payload[k] for k in todo], [ents[k].usize for k in todo], deliver=not test_only))
        todo = [k for k in range(len(ents)) if k not in res and ents[k].method == 14]
        if todo:
            settle(todo, self.enc.unlzma_batch([payload[k] for k in todo], [ents[k].usize for k in todo], [bool(ents[k].flags & 2) for k in todo], deliver=not test_only))
        todo = [k for k in range(len(ents)) if k not in res and 1 <= ents[k].method <= 6]
        if todo:
            settle(todo, self.enc.unlegacy_batch([payload[k] for k in todo], [ents[k].usize for k in todo], [ents[k].method for k in todo],
                                                 [ents[k].flags & 6 for k in todo], deliver=not test_only))
        for k, e in enumerate(ents):
            if k in res:
                continue
            d = payload[k]                                 # Store: the slice itself
            ex = self._verdict(e, 0, len(d), (zlib.crc32(d) & 0xFFFFFFFF) ^ 0xFFFFFFFF)
            res[k] = ex if ex is not None else None if test_only else d
        return self._finish(ents, res, test_only, errors)

    def _deflate64_knob(self, back=None):
        """parallel_deflate64=True: sets the knob "inflate_par_deflate64" and returns the value it had; with that value, puts it back."""
        if not self.parallel_deflate64:
            return None
        if back is None:
            back = getattr(self.enc, "_knobs_set", {}).get("inflate_par_deflate64", 0)
            self.enc.set_knob("inflate_par_deflate64", 1)
            return back
        self.enc.set_knob("inflate_par_deflate64", back)

    def _batch_knob(self, back=None):
        """parallel_batch=True: sets the knob "inflate_par_batch" and returns the value it had; with that value, puts it back."""
        if not self.parallel_batch:
            return None
        if back is None:
            back = getattr(self.enc, "_knobs_set", {}).get("inflate_par_batch", 0)
            self.enc.set_knob("inflate_par_batch", 1)
            return back
        self.enc.set_knob("inflate_par_batch", back)

    def extract_device(self, info, what=None, password=None, test_only=False, errors="raise"):
        """extract for an archive that lies in device memory: info is a ZipInfo.load_device of a tensor on the encoder's device.  Returns
        {name: torch.uint8 tensor} -- views of ONE output tensor, every entry at a multiple of 256 bytes --, with what, password, test_only, errors, the
        exceptions and their .results as extract has them.  One zada_unzip_device call takes all entries the reader decodes: no entry byte crosses the
        host, encrypted entries are decoded on the device, stored ones copied and summed there (the device's CRC-32 is what is compared with the
        directory).  An empty selection makes no device call."""
        import numpy as np
        import torch
        t = info.device_data
        if t is None:
            raise ZadaError("UnZip.extract_device: the ZipInfo was not made by ZipInfo.load_device")
        ents = info.entries if what is None else [info[nm] for nm in ([what] if isinstance(what, str) else what)]
        res, rows = {}, []
        for k, e in enumerate(ents):
            ex = self._unsupported(e)
            if ex is None and e.encrypted:
                if password is None:
                    ex = WrongPassword("entry %r is encrypted and no password was given" % e.name)
                elif e.csize < 12:
                    ex = DataError("entry %r: shorter than its encryption header" % e.name)
            if ex is not None:
                res[k] = ex
            else:
                rows.append(k)
        if rows:
            if t.device.type != "cuda" or t.device.index != self.enc.device:
                raise ZadaError("UnZip.extract_device: the archive tensor lies on %s, not on the encoder's device" % t.device)
            # the table, column by column (ten thousand rows are a few milliseconds this way)
            n = len(rows)
            E = [ents[k] for k in rows]
            col = lambda f, dt=np.uint64: np.fromiter((f(e) for e in E), dt, n)
            crypt, method, usize = col(lambda e: e.encrypted, np.uint8), col(lambda e: e.method, np.uint16), col(lambda e: e.usize)
            tab = np.zeros(n, dtype=self.enc.unzip_dtypes()[0])
            tab["in_off"], tab["n_in"], tab["method"] = col(lambda e: e.data_offset), col(lambda e: e.csize), method
            # (a stored entry gets room for what is stored: whether that is what the directory promises is the verdict's to say, behind the password's)
            tab["cap"] = np.where(method == 0, tab["n_in"] - crypt * np.uint64(12), usize)
            slots = (tab["cap"] + np.uint64(255)) & ~np.uint64(255)
            tab["out_off"] = np.cumsum(slots) - slots
            total = int(slots.sum())
            tab["flags"] = crypt | col(lambda e: e.flags & (6 if e.method == 6 else 2), np.uint8)
            # the header's last byte (zip-compress.adb:153-161; bit 3: the time stamp)
            tab["check"] = col(lambda e: ((e.dos_time >> 8) if e.flags & 8 else (e.crc >> 24)) & 0xFF, np.uint8)
            out = None if test_only else torch.empty(max(total, 1), dtype=torch.uint8, device=t.device)
            keys0 = self.enc.crypt_init_keys(password) if password is not None and crypt.any() else None
            torch.cuda.current_stream(t.device).synchronize()
            if self.parallel_inflate is not None:
                self.enc.set_knob("inflate_par_min_kib", self.parallel_inflate)
            was = self._deflate64_knob()
            was_batch = self._batch_knob()
            if self.legacy:
                self.enc.set_knob("unzip_legacy", 1)
            try:
                _, r = self.enc.unzip_device(t.data_ptr(), t.numel(), None if out is None else out.data_ptr(), 0 if out is None else total, tab, keys0)
            finally:
                if self.parallel_inflate is not None:
                    self.enc.set_knob("inflate_par_min_kib", 0)
                self._deflate64_knob(was)
                self._batch_knob(was_batch)
                if self.legacy:
                    self.enc.set_knob("unzip_legacy", 0)
            good = (r["rc"] == 0) & (r["out_len"] == usize) & ((r["crc"] ^ np.uint32(0xFFFFFFFF)) == col(lambda e: e.crc, np.uint32))
            if out is not None:                                # every good entry's view in one split: cuts in front of and behind each
                cuts = np.stack((tab["out_off"], tab["out_off"] + np.where(good, usize, 0).astype(np.uint64)), axis=1).reshape(-1)
                views = out.tensor_split([int(x) for x in cuts])[1::2]
            for j, k in enumerate(rows):
                if good[j]:
                    res[k] = None if test_only else views[j]
                elif r["rc"][j] == E_PASSWORD:
                    res[k] = WrongPassword("entry %r: wrong password" % E[j].name)
                else:
                    res[k] = self._verdict(E[j], int(r["rc"][j]), int(r["out_len"][j]), int(r["crc"][j]))
        return self._finish(ents, res, test_only, errors)


CZ_OK, CZ_DIFFERENT, CZ_SHORTER, CZ_LONGER, CZ_MISSING, CZ_DAMAGED = range(6)      # zada_compzip_result.verdict
CZ_ABSENT = 0x80                                                                    # zada_unzip_entry.flags: archive 2 has no entry of that name


class CompZipResult:
    """What Comp_Zip_Prc counts (comp_zip_prc.adb:27-35, 158-172): total_1, total_2, common, size_failures, compare_failures, missing_1_in_2,
    just_a_directory, missing_2_in_1, total_bytes and total_differences = size_failures + compare_failures + missing_1_in_2 + missing_2_in_1 +
    damaged.  damaged counts the pairs of which a side did not decode or did not meet its directory's size and CRC-32: the reference ends with the
    reader's exception there, this one goes on and counts them as differences.
    entries: per entry of archive 1, in the order of the traversal, (name, verdict, position, compared, error, key) -- verdict one of CZ_*, position
    the 1-based position of CZ_DIFFERENT / CZ_SHORTER, compared the equal bytes in front of the verdict, error the exception of a CZ_DAMAGED pair, key
    the name the tool goes by: the raw name's bytes with '\\' turned into '/'.  result [x] finds an entry by its key (bytes) or its display name."""
    _COUNTERS = ("total_1", "total_2", "common", "size_failures", "compare_failures", "missing_1_in_2", "just_a_directory", "missing_2_in_1", "damaged",
                 "total_bytes", "total_differences")

    def __init__(self):
        for nm in self._COUNTERS:
            setattr(self, nm, 0)
        self.entries = []

    def __getitem__(self, name):
        for e in self.entries:
            if e[5 if isinstance(name, bytes) else 0] == name:
                return e
        raise KeyError(name)

    def __repr__(self):
        return "CompZipResult(%s)" % ", ".join("%s=%d" % (nm, getattr(self, nm)) for nm in self._COUNTERS)


def zip_load_order(info, who="Zip.Load"):
    """The entries of a ZipInfo in the order Zip.Traverse visits them: ascending by the raw name with '\\' turned into '/', compared byte by byte
    (Normalize and Insert_into_tree, zip.adb:152-166, 195-237, case-sensitive) -- as [(key, ZipEntry)].  Two entries with the same key raise, as Load's
    error_on_duplicate does."""
    rows = sorted(((e.raw_name.replace(b"\\", b"/"), k, e) for k, e in enumerate(info.entries)), key=lambda r: (r[0], r[1]))
    for x, y in zip(rows, rows[1:]):
        if x[0] == y[0]:
            raise ZadaError("%s: the same full entry name (%r) appears twice in the archive's directory" % (who, x[2].name))
    return [(r[0], r[2]) for r in rows]


class CompZip:
    """Comp_Zip_Prc (tools/comp_zip_prc.adb) on two archives that lie in device memory: every entry of archive 1, in Zip.Traverse's order, is looked up
    by name in archive 2 (case-sensitive, '\\' = '/'), both are extracted on the device and compared there (zada_compzip_device); no entry byte
    crosses the host.  Every method the reader decodes takes part (Store, Deflate, Deflate64, BZip2, LZMA; with legacy=True also Shrink, Reduce and
    Implode); any other raises UnsupportedMethod in UnZip's words, an encrypted entry without a password WrongPassword."""

    def __init__(self, encoder, legacy=False):
        self.enc = encoder
        self.legacy = bool(legacy)

    def compare_device(self, info1, info2, password=None):
        """info1, info2: ZipInfo.load_device of two tensors on the encoder's device; password: of both archives.  -> CompZipResult"""
        import numpy as np
        import torch
        t1, t2 = info1.device_data, info2.device_data
        if t1 is None or t2 is None:
            raise ZadaError("CompZip.compare_device: the ZipInfos were not made by ZipInfo.load_device")
        for t in (t1, t2):
            if t.device.type != "cuda" or t.device.index != self.enc.device:
                raise ZadaError("CompZip.compare_device: an archive tensor lies on %s, not on the encoder's device" % t.device)
        order1 = zip_load_order(info1, "CompZip.compare_device (archive 1)")
        dir2 = dict(zip_load_order(info2, "CompZip.compare_device (archive 2)"))
        reader = UnZip(self.enc, bzip2=True, lzma=True, legacy=self.legacy)
        pairs = [(key, e, dir2.get(key)) for key, e in order1]
        for _, e1, e2 in pairs:
            for e in (e1, e2) if e2 is not None else (e1,):        # (the C call looks at every row of archive 1, the missing pairs' too)
                ex = reader._unsupported(e)
                if ex is None and e.encrypted and password is None:
                    ex = WrongPassword("entry %r is encrypted and no password was given" % e.name)
                if ex is not None:
                    raise ex
        n = len(pairs)
        dt = self.enc.unzip_dtypes()[0]

        def table(ents):
            # column by column, as in UnZip.extract_device; a missing entry is a row of zeros with CZ_ABSENT
            col = lambda f, dt=np.uint64: np.fromiter((0 if e is None else f(e) for e in ents), dt, n)
            tab = np.zeros(n, dtype=dt)
            crypt, method = col(lambda e: e.encrypted, np.uint8), col(lambda e: e.method, np.uint16)
            tab["in_off"], tab["n_in"], tab["method"] = col(lambda e: e.data_offset), col(lambda e: e.csize), method
            # (a stored entry gets room for what is stored, as there)
            tab["cap"] = np.where(method == 0, col(lambda e: max(e.csize - 12, 0) if e.encrypted else e.csize), col(lambda e: e.usize))
            tab["flags"] = crypt | col(lambda e: e.flags & (6 if e.method == 6 else 2), np.uint8) | np.fromiter((CZ_ABSENT if e is None else 0 for e in ents), np.uint8, n)
            tab["check"] = col(lambda e: ((e.dos_time >> 8) if e.flags & 8 else (e.crc >> 24)) & 0xFF, np.uint8)
            return tab
        out = CompZipResult()
        out.total_2 = len(info2.entries)
        if n:
            keys0 = self.enc.crypt_init_keys(password) if password is not None else None
            torch.cuda.current_stream(t1.device).synchronize()
            if self.legacy:
                self.enc.set_knob("unzip_legacy", 1)
            try:
                r = self.enc.compzip_device(t1.data_ptr(), t1.numel(), t2.data_ptr(), t2.numel(), table([p[1] for p in pairs]), table([p[2] for p in pairs]), keys0)
            finally:
                if self.legacy:
                    self.enc.set_knob("unzip_legacy", 0)
        for k, (key, e1, e2) in enumerate(pairs):
            out.total_1 += 1
            v, pos, cmpd, err = int(r["verdict"][k]), int(r["position"][k]), int(r["compared"][k]), None
            if v == CZ_MISSING:
                if key[-1:] == b"/":                       # (the traversal's names have no '\\' left)
                    out.just_a_directory += 1
                out.missing_1_in_2 += 1
            else:
                for e, side in ((e1, "a"), (e2, "b")):
                    rc = int(r["rc_" + side][k])
                    ex = WrongPassword("entry %r: wrong password" % e.name) if rc == E_PASSWORD else reader._verdict(e, rc, int(r["len_" + side][k]), int(r["crc_" + side][k]))
                    if ex is not None and err is None:
                        err = ex
                if err is not None:
                    v, pos, cmpd = CZ_DAMAGED, 0, 0
                    out.damaged += 1
                elif v in (CZ_SHORTER, CZ_LONGER):
                    out.size_failures += 1
                elif v == CZ_DIFFERENT:
                    out.compare_failures += 1
                else:
                    out.total_bytes += cmpd
            out.entries.append((e1.name, v, pos, cmpd, err, key))
        out.common = out.total_1 - out.missing_1_in_2
        out.missing_2_in_1 = out.total_2 - out.common
        out.total_differences = out.size_failures + out.compare_failures + out.missing_1_in_2 + out.missing_2_in_1 + out.damaged
        return out


class ReZip:
    """ReZip (tools/rezip_lib.adb, `rezip -int`) on an archive that lies in device memory: every entry is extracted and compressed on the device with
    each considered approach, and the new archive keeps per entry the smallest stream, the source's own where nothing beats it (zada_rezip_device).
    legacy=True: the approaches shrink and reduce_4, which the reference tries on entries of at most 6 000 and 9 000 bytes, are taken, approaches=None
    then means all twelve, and source entries of methods 1 .. 6 (Shrink, Reduce, Implode) are read (the knobs "zip_legacy" and "unzip_legacy" are set
    around the call).  The C format mask cannot name the formats of these methods: they count as in the format set exactly when the set is "all".
    Without legacy=True the two approaches and such sources are refused by name.
    Divergences from the reference: an LZMA_3 entry the coder refuses loses that approach instead of getting a stream that does not decode; more than 65 534
    kept entries are refused; the headers carry the directory's CRC-32; with lower=True two names that differ only in case are refused as duplicates,
    where the reference writes both; a kept Implode stream keeps general-purpose bits 1 and 2 of its source, which the reference's mask 0xFFF5 would
    cut to bit 2 alone (its own output then no longer decodes)."""
    _FORMATS = {"all": RZ_ALL_FORMATS, "deflate_or_store": RZ_DEFLATE_OR_STORE, "fast_decompression": RZ_FAST_DECOMPRESSION}

    def __init__(self, encoder, legacy=False):
        self.enc = encoder
        self.legacy = bool(legacy)

    def rezip_device(self, info, formats="all", approaches=None, touch=None, lower=False, delete_comment=False, report=False):
        """info: ZipInfo.load_device of a tensor on the encoder's device.  formats: "all", "deflate_or_store", "fast_decompression" or a bit set;
        approaches: None (the default ten; with legacy=True all twelve), a bit mask, or names of RZ_APPROACHES; touch: one DOS time stamp for all entries; lower: names in lower
        case; delete_comment: the archive comment is left out.  Entries are written in Zip.Load's order (zip_load_order; a duplicate raises).
        Returns the new archive as a torch.uint8 tensor on the device, or (tensor, report) with report = {"entries": [(name, {approach: size},
        choice)], "totals": {approach: {"count": wins, "saved": bytes saved against original}}}."""
        import numpy as np
        import torch
        t = info.device_data
        if t is None:
            raise ZadaError("ReZip.rezip_device: the ZipInfo was not made by ZipInfo.load_device")
        if t.device.type != "cuda" or t.device.index != self.enc.device:
            raise ZadaError("ReZip.rezip_device: the archive tensor lies on %s, not on the encoder's device" % t.device)
        fmt = self._FORMATS[formats] if isinstance(formats, str) else int(formats)
        if approaches is None:
            mask = RZ_DEFAULT | (RZ_LEGACY if self.legacy else 0)
        elif isinstance(approaches, int):
            mask = approaches
        else:
            mask = 0
            for a in approaches:
                mask |= 1 << RZ_APPROACHES.index(a)
        order = zip_load_order(info, "ReZip.rezip_device")
        reader = UnZip(self.enc, bzip2=True, lzma=True, legacy=self.legacy)
        for _, e in order:
            ex = reader._unsupported(e)
            if ex is not None:
                raise ex
        names = [(key.decode("latin-1").lower().encode("latin-1") if lower else key) for key, _ in order]
        n = len(order)
        dt = self.enc.rezip_dtypes()[0]
        tab = np.zeros(n, dtype=dt)
        blob = np.frombuffer(b"".join(names) + b"\0", dtype=np.uint8)
        E = [e for _, e in order]
        col = lambda f, d=np.uint64: np.fromiter((f(e) for e in E), d, n)
        nlen = np.fromiter((len(nm) for nm in names), np.uint64, n)
        tab["in_off"], tab["n_in"], tab["usize"], tab["crc"] = col(lambda e: e.data_offset), col(lambda e: e.csize), col(lambda e: e.usize), col(lambda e: e.crc, np.uint32)
        tab["time"] = col(lambda e: e.local_time, np.uint32) if touch is None else touch
        tab["method"], tab["flags"], tab["version"] = col(lambda e: e.method, np.uint16), col(lambda e: e.local_flags, np.uint16), col(lambda e: e.local_version, np.uint16)
        tab["name_len"], tab["name"] = nlen, np.uint64(blob.ctypes.data) + np.cumsum(nlen) - nlen
        comment = b"" if delete_comment else bytes(info.comment)
        cap = self.enc.rezip_bound(tab, len(comment))
        out = torch.empty(cap, dtype=torch.uint8, device=t.device)
        torch.cuda.current_stream(t.device).synchronize()
        if self.legacy:
            self.enc.set_knob("zip_legacy", 1)
            self.enc.set_knob("unzip_legacy", 1)
        try:
            alen, res, sizes = self.enc.rezip_device(t.data_ptr(), t.numel(), tab, out.data_ptr(), cap, mask, fmt, 0, comment)
        finally:
            if self.legacy:
                self.enc.set_knob("zip_legacy", 0)
                self.enc.set_knob("unzip_legacy", 0)
        if not report:
            return out[:alen]
        rep = {"entries": [], "totals": {a: {"count": 0, "saved": 0} for a in RZ_APPROACHES}}
        for k, nm in enumerate(names):
            if res["flags"][k] & 1:
                continue
            row = {a: int(sizes[k][j]) for j, a in enumerate(RZ_APPROACHES) if int(sizes[k][j]) != RZ_NOT_TRIED}
            choice = RZ_APPROACHES[int(res["approach"][k])]
            rep["entries"].append((nm, row, choice))
            rep["totals"][choice]["count"] += 1
            rep["totals"][choice]["saved"] += row["original"] - row[choice]
        return out[:alen], rep

    def rezip(self, archive_bytes, **kw):
        """rezip_device for an archive in host bytes: -> bytes, or (bytes, report)."""
        import numpy as np
        import torch
        t = torch.from_numpy(np.frombuffer(bytes(archive_bytes), dtype=np.uint8).copy()).to(torch.device("cuda", self.enc.device))
        r = self.rezip_device(ZipInfo.load_device(t), **kw)
        if isinstance(r, tuple):
            return r[0].cpu().numpy().tobytes(), r[1]
        return r.cpu().numpy().tobytes()


_L1_UPPER = bytes(c - 0x20 if 0x61 <= c <= 0x7A or 0xE0 <= c <= 0xF6 or 0xF8 <= c <= 0xFE else c for c in range(256))      # Ada.Characters.Handling.To_Upper
_L1_LOWER = bytes(c + 0x20 if 0x41 <= c <= 0x5A or 0xC0 <= c <= 0xD6 or 0xD8 <= c <= 0xDE else c for c in range(256))      # ... To_Lower


class FindZipResult:
    """What Find_Zip reports (tools/find_zip.adb).  entries: per entry of the archive, in the order of the traversal, (name, occurrences, first,
    error, key) -- occurrences what the loop of find_zip.adb:64-84 counts in the entry's decoded bytes, first the 0-based offset of the last byte of
    the first occurrence (the entry's length where there is none), error the reader's exception for an entry that did not decode or did not meet its
    size and CRC-32 (occurrences and first are then 0), key the name the tool goes by: the raw name's bytes with '\\' turned into '/'.
    in_contents: [(key, occurrences)] with occurrences > 0; in_names: the keys that contain the string; damaged: how many entries carry an error --
    the reference ends with the reader's exception at the first of them, this one goes on.  result [x] finds an entry by its key (bytes) or its
    display name."""

    def __init__(self):
        self.entries, self.in_contents, self.in_names, self.damaged = [], [], [], 0

    def __getitem__(self, name):
        for e in self.entries:
            if e[4 if isinstance(name, bytes) else 0] == name:
                return e
        raise KeyError(name)

    def lines(self):
        """The reference's output between "Searching string" and "Time elapsed", line by line: Put (occ, 5) and the name in lower case for every
        entry whose contents hold the string, then every name that holds it."""
        low = lambda key: key.translate(_L1_LOWER).decode("latin-1")
        return (["%5d in [%s]'s contents" % (occ, low(key)) for key, occ in self.in_contents] +
                [" Found in [%s]'s entry name" % low(key) for key in self.in_names])

    def __repr__(self):
        return "FindZipResult(in_contents=%d, in_names=%d, damaged=%d)" % (len(self.in_contents), len(self.in_names), self.damaged)


class FindZip:
    """Find_Zip (tools/find_zip.adb) on an archive that lies in device memory: every entry, in Zip.Traverse's order, is extracted on the device and
    searched there for a string (zada_findzip_device); no entry byte crosses the host.  The names are searched on the host.  Every method the reader
    decodes takes part (Store, Deflate, Deflate64, BZip2, LZMA; with legacy=True also Shrink, Reduce and Implode); any other raises UnsupportedMethod
    in UnZip's words, an encrypted entry without a password WrongPassword."""

    def __init__(self, encoder, legacy=False):
        self.enc = encoder
        self.legacy = bool(legacy)

    def find_device(self, info, text, ignore_case=True, password=None):
        """info: ZipInfo.load_device of a tensor on the encoder's device; text: bytes, or a str taken as Latin-1 (1 .. 1024 bytes, else ValueError);
        ignore_case: the reference's constant, True; password: the archive's.  -> FindZipResult"""
        import numpy as np
        import torch
        text = _search_text(text)
        t = info.device_data
        if t is None:
            raise ZadaError("FindZip.find_device: the ZipInfo was not made by ZipInfo.load_device")
        if t.device.type != "cuda" or t.device.index != self.enc.device:
            raise ZadaError("FindZip.find_device: the archive tensor lies on %s, not on the encoder's device" % t.device)
        order = zip_load_order(info, "FindZip.find_device")
        reader = UnZip(self.enc, bzip2=True, lzma=True, legacy=self.legacy)
        for _, e in order:
            ex = reader._unsupported(e)
            if ex is None and e.encrypted and password is None:
                ex = WrongPassword("entry %r is encrypted and no password was given" % e.name)
            if ex is not None:
                raise ex
        n = len(order)
        E = [e for _, e in order]
        out = FindZipResult()
        if n:
            # the table, column by column, as in UnZip.extract_device (a stored entry gets room for what is stored)
            col = lambda f, dt=np.uint64: np.fromiter((f(e) for e in E), dt, n)
            tab = np.zeros(n, dtype=self.enc.unzip_dtypes()[0])
            crypt, method = col(lambda e: e.encrypted, np.uint8), col(lambda e: e.method, np.uint16)
            tab["in_off"], tab["n_in"], tab["method"] = col(lambda e: e.data_offset), col(lambda e: e.csize), method
            tab["cap"] = np.where(method == 0, col(lambda e: max(e.csize - 12, 0) if e.encrypted else e.csize), col(lambda e: e.usize))
            tab["flags"] = crypt | col(lambda e: e.flags & (6 if e.method == 6 else 2), np.uint8)
            tab["check"] = col(lambda e: ((e.dos_time >> 8) if e.flags & 8 else (e.crc >> 24)) & 0xFF, np.uint8)
            keys0 = self.enc.crypt_init_keys(password) if password is not None else None
            torch.cuda.current_stream(t.device).synchronize()
            if self.legacy:
                self.enc.set_knob("unzip_legacy", 1)
            try:
                r = self.enc.findzip_device(t.data_ptr(), t.numel(), tab, text, ignore_case, keys0)
            finally:
                if self.legacy:
                    self.enc.set_knob("unzip_legacy", 0)
        for k, (key, e) in enumerate(order):
            rc = int(r["rc"][k])
            err = WrongPassword("entry %r: wrong password" % e.name) if rc == E_PASSWORD else reader._verdict(e, rc, int(r["out_len"][k]), int(r["crc"][k]))
            occ, first = (0, 0) if err is not None else (int(r["occurrences"][k]), int(r["first"][k]))
            out.damaged += err is not None
            out.entries.append((e.name, occ, first, err, key))
            if occ > 0:
                out.in_contents.append((key, occ))
        # Search_in_entry_name (find_zip.adb:150-159), on the host: Index (To_Upper (name), str) > 0
        s = text.translate(_L1_UPPER) if ignore_case else text
        out.in_names = [key for key, _ in order if (key.translate(_L1_UPPER) if ignore_case else key).find(s) >= 0]
        return out

    def find(self, archive_bytes, text, **kw):
        """find_device for an archive in host bytes."""
        import numpy as np
        import torch
        t = torch.from_numpy(np.frombuffer(bytes(archive_bytes), dtype=np.uint8).copy()).to(torch.device("cuda", self.enc.device))
        return self.find_device(ZipInfo.load_device(t), text, **kw)


class TrainedCompression:
    """Trained_Compression (trained/trained_compression.ads) for batches of messages: every message is the tail of one LZMA stream (Level_3, lc 3,
    lp 0, pb 2, dictionary 2 ** 19) whose head is training data both sides know (include/zada.h).

    TrainedCompression (encoder, trainer, skip=None, noise=b"") is the ENCODING side: `trainer` is bytes or a torch.uint8 tensor, `noise` is appended
    to it (as trtest_single.cmd appends rnd_10.bin).  .stub is Encode_Trainer's output, the compressed trainer the decoding side keeps; .skip the
    stream bytes every message leaves out; skip=None means max (0, len (stub) - 140), the calibration of trtest_single.cmd -- the caller answers
    for a skip that is no longer than what the streams have in common.  .trainer_len counts the noise.
    TrainedCompression.for_decoding (encoder, stub, skip, trainer_len) is the DECODING side: it has the stub, not the trainer."""
    SKIP_MARGIN = 140          # trtest_single.cmd: skip = the stub's length less this
    _ENTRY = [("d_data", "<u8"), ("n", "<u8"), ("d_out", "<u8"), ("cap", "<u8")]
    _INFO = ("fork_pos", "fork_out", "dec_fork_in", "dec_fork_out", "forked", "unforked")

    def __init__(self, encoder, trainer, skip=None, noise=b""):
        self.enc, self.h, self.side = encoder, None, "encode"
        t = bytes(trainer.cpu().numpy().tobytes()) if hasattr(trainer, "data_ptr") else bytes(trainer)
        t += bytes(noise)
        self.trainer_len = len(t)
        L = encoder.lib
        cap = len(t) + len(t) // 8 + 4096
        out = ctypes.create_string_buffer(cap)
        ol = ctypes.c_uint64()
        rc = L.zada_trained_stub(encoder.ctx, t, len(t), out, cap, ctypes.byref(ol))
        if rc != 0:
            encoder._err(rc, "zada_trained_stub")
        self.stub = out.raw[:ol.value]
        self.skip = max(0, len(self.stub) - self.SKIP_MARGIN) if skip is None else int(skip)
        h = ctypes.c_void_p()
        rc = L.zada_trained_open_encoder(encoder.ctx, t, len(t), 0, self.skip, ctypes.byref(h))
        if rc != 0:
            encoder._err(rc, "zada_trained_open_encoder")
        self.h = h

    @classmethod
    def for_decoding(cls, encoder, stub, skip, trainer_len):
        self = cls.__new__(cls)
        self.enc, self.h, self.side = encoder, None, "decode"
        self.stub, self.skip, self.trainer_len = bytes(stub), int(skip), int(trainer_len)
        h = ctypes.c_void_p()
        rc = encoder.lib.zada_trained_open_decoder(encoder.ctx, self.stub, len(self.stub), self.skip, self.trainer_len, ctypes.byref(h))
        if rc != 0:
            encoder._err(rc, "zada_trained_open_decoder")
        self.h = h
        return self

    def close(self):
        if getattr(self, "h", None):
            self.enc.lib.zada_trained_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        """fork_pos / fork_out (encoder: trainer positions coded once and stream bytes written there), dec_fork_in / dec_fork_out (decoder: stub bytes taken
        and trainer bytes written once), forked / unforked: entries of the last call that started from the snapshot / that ran their whole stream."""
        v = (ctypes.c_uint64 * 6)()
        if self.enc.lib.zada_trained_info(self.h, v) != 0:
            raise ZadaError("zada_trained_info failed")
        return dict(zip(self._INFO, (int(x) for x in v)))

    def _call(self, fn, rows):
        """rows: (d_data, n, d_out, cap) per entry -> (the call's rc, out_len per entry, rc per entry)."""
        import numpy as np
        tab = np.array([tuple(int(x) for x in r) for r in rows], dtype=self._ENTRY) if rows else np.zeros(0, dtype=self._ENTRY)
        n = len(tab)
        ol, rcs = np.zeros(max(n, 1), np.uint64), np.full(max(n, 1), 99, np.int32)
        rc = fn(self.enc.ctx, self.h, n, tab.ctypes.data if n else None, ol.ctypes.data, rcs.ctypes.data)
        return rc, [int(x) for x in ol[:n]], [int(x) for x in rcs[:n]]

    def encode_raw(self, rows):
        """zada_trained_encode_device on device addresses: rows of (d_data, n, d_out, cap) -> (rc, out_len [], rc [])."""
        return self._call(self.enc.lib.zada_trained_encode_device, rows)

    def decode_raw(self, rows):
        """zada_trained_decode_device on device addresses: rows of (d_msg, n_msg, d_out, cap) -> (rc, out_len [], rc [])."""
        return self._call(self.enc.lib.zada_trained_decode_device, rows)

    def _tensors(self, items, who):
        import numpy as np
        import torch
        dev = torch.device("cuda", self.enc.device)
        out = []
        for t in items:
            if not isinstance(t, torch.Tensor):
                b = bytes(t)
                t = torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).to(dev) if b else torch.empty(0, dtype=torch.uint8, device=dev)
            if t.dtype != torch.uint8 or not t.is_contiguous() or (t.numel() and t.device != dev):
                raise ZadaError("%s: contiguous torch.uint8 tensors on %s are needed" % (who, dev))
            out.append(t)
        return out, dev

    def encode_device(self, datas):
        """One message per data tensor (contiguous torch.uint8 on the encoder's device), in ONE call: the bytes Trained_Compression.Encode writes
        for trainer & data with Skip_Compressed = skip.  Returns tensors on the device.  ReferenceDefect as Encoder.lzma_batch."""
        import torch
        datas, dev = self._tensors(datas, "TrainedCompression.encode_device")
        caps = [t.numel() + t.numel() // 8 + self.SKIP_MARGIN + 256 for t in datas]         # (what is left of the stub behind skip, the data, the marker)
        for attempt in range(2):
            outs = [torch.empty(c, dtype=torch.uint8, device=dev) for c in caps]
            torch.cuda.current_stream(dev).synchronize()
            rc, ols, rcs = self.encode_raw([(t.data_ptr() if t.numel() else 0, t.numel(), o.data_ptr(), c) for t, o, c in zip(datas, outs, caps)])
            if rc == 0:
                return [o[:n] for o, n in zip(outs, ols)]
            if attempt == 0 and all(r == 0 or (r == -1 and n > c) for r, n, c in zip(rcs, ols, caps)):
                caps = [max(c, n) for c, n in zip(caps, ols)]                                  # (a skip far below the stub's length: the lengths are known now)
                continue
            self.enc._err(rc, "zada_trained_encode_device")

    def encode(self, datas):
        """encode_device for data in host bytes -> list of bytes."""
        return [bytes(t.cpu().numpy().tobytes()) for t in self.encode_device(datas)]

    def decode_device(self, messages, caps, errors="raise"):
        """One data tensor per message (bytes or contiguous torch.uint8 tensors on the encoder's device), caps [i] bytes of room each, in ONE call:
        what Trained_Compression.Decode writes for stub [0 .. skip) & message.  A message that is no valid stream, or holds more than caps [i]
        bytes, raises DataError naming the first such entry; errors="return" puts a DataError in its place instead."""
        import torch
        msgs, dev = self._tensors(messages, "TrainedCompression.decode_device")
        caps = [int(c) for c in caps]
        if len(caps) != len(msgs):
            raise ValueError("TrainedCompression.decode_device: %d caps for %d messages" % (len(caps), len(msgs)))
        outs = [torch.empty(c, dtype=torch.uint8, device=dev) for c in caps]
        torch.cuda.current_stream(dev).synchronize()
        rc, ols, rcs = self.decode_raw([(t.data_ptr() if t.numel() else 0, t.numel(), o.data_ptr() if c else 0, c) for t, o, c in zip(msgs, outs, caps)])
        if rc != 0 and (rc != E_DATA or errors != "return"):
            self.enc._err(rc, "zada_trained_decode_device")
        return [o[:n] if r == 0 else DataError("trained decode: entry %d is not a valid stream for this stub" % k) for k, (o, n, r) in enumerate(zip(outs, ols, rcs))]

    def decode(self, messages, caps, errors="raise"):
        """decode_device -> list of bytes."""
        return [r if isinstance(r, Exception) else bytes(r.cpu().numpy().tobytes()) for r in self.decode_device(messages, caps, errors)]
