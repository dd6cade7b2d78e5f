// UNVERIFIED (no .NET SDK in the build image).  The compressor the reference declares only in a comment
// (csharp/src/ZStd.cs:89-96 Compress, :144-145 ZSTD_COMPRESSBOUND, :146-148 IsError / GetErrorName), over libzsmi.so.
using System;
using System.Runtime.InteropServices;

namespace EPAM.Deltix.ZStd
{
    public static unsafe class ZStdCompress
    {
        [DllImport(ZStdDecompress.Lib, CallingConvention = CallingConvention.Cdecl)]
        static extern UIntPtr zsmi_compress(void* dst, UIntPtr dstCapacity, void* src, UIntPtr srcSize, int level);
        [DllImport(ZStdDecompress.Lib, CallingConvention = CallingConvention.Cdecl)]
        static extern UIntPtr zsmi_compressBound(UIntPtr srcSize);
        [DllImport(ZStdDecompress.Lib, CallingConvention = CallingConvention.Cdecl)]
        static extern UIntPtr zsmi_compress_usingDict(void* dst, UIntPtr dstCapacity, void* src, UIntPtr srcSize, void* dict, UIntPtr dictSize, int level);
        [DllImport(ZStdDecompress.Lib, CallingConvention = CallingConvention.Cdecl)]
        static extern UIntPtr zsmi_compress_advanced(void* dst, UIntPtr dstCapacity, void* src, UIntPtr srcSize, void* dict, UIntPtr dictSize, int level, int checksumFlag);
        [DllImport(ZStdDecompress.Lib, CallingConvention = CallingConvention.Cdecl)]
        static extern IntPtr zsmi_getErrorName(UIntPtr code);

        public const int DefaultLevel = 3;

        public static uint CompressBound(uint srcSize) => (uint)zsmi_compressBound((UIntPtr)srcSize);

        // one frame for the whole input; returns the frame size or (uint)(-code)
        public static uint Compress(byte[] dst, uint dstCapacity, byte[] src, uint srcSize, int compressionLevel = DefaultLevel)
        {
            if (dst == null || src == null) throw new ArgumentNullException(dst == null ? nameof(dst) : nameof(src));
            if (dstCapacity > (uint)dst.Length || srcSize > (uint)src.Length) throw new ArgumentOutOfRangeException();
            fixed (byte* d = dst, s = src)
                return unchecked((uint)(ulong)zsmi_compress(d, (UIntPtr)dstCapacity, s, (UIntPtr)srcSize, compressionLevel));
        }
        // the same with a dictionary (raw content or formatted, as ZStdDecompress's usingDict decode takes it); null / empty = Compress
        public static uint CompressUsingDict(byte[] dst, uint dstCapacity, byte[] src, uint srcSize, byte[] dict, int compressionLevel = DefaultLevel)
        {
            if (dst == null || src == null) throw new ArgumentNullException(dst == null ? nameof(dst) : nameof(src));
            if (dstCapacity > (uint)dst.Length || srcSize > (uint)src.Length) throw new ArgumentOutOfRangeException();
            fixed (byte* d = dst, s = src, dc = dict)
                return unchecked((uint)(ulong)zsmi_compress_usingDict(d, (UIntPtr)dstCapacity, s, (UIntPtr)srcSize, dc, (UIntPtr)(uint)(dict?.Length ?? 0), compressionLevel));
        }
        // the same with a content checksum (ZSTD_c_checksumFlag): the frame of Compress / CompressUsingDict with bit 2 of byte 4 set and the low 32 bits
        // of the content's XXH64 behind the last block; a decoder answers checksum_wrong (22) for a frame whose content it cannot restore.
        // dict: null / empty = none; checksum false: Compress / CompressUsingDict byte for byte
        public static uint Compress(byte[] dst, uint dstCapacity, byte[] src, uint srcSize, byte[] dict, int compressionLevel, bool checksum)
        {
            if (dst == null || src == null) throw new ArgumentNullException(dst == null ? nameof(dst) : nameof(src));
            if (dstCapacity > (uint)dst.Length || srcSize > (uint)src.Length) throw new ArgumentOutOfRangeException();
            fixed (byte* d = dst, s = src, dc = dict)
                return unchecked((uint)(ulong)zsmi_compress_advanced(d, (UIntPtr)dstCapacity, s, (UIntPtr)srcSize, dc, (UIntPtr)(uint)(dict?.Length ?? 0), compressionLevel, checksum ? 1 : 0));
        }
        public static uint Compress(byte[] dst, byte[] src, int compressionLevel = DefaultLevel) => Compress(dst, (uint)dst.Length, src, (uint)src.Length, compressionLevel);

        public static byte[] Compress(byte[] src, int compressionLevel = DefaultLevel)
        {
            var dst = new byte[CompressBound((uint)src.Length)];
            uint r = Compress(dst, src, compressionLevel);
            if (ZStdDecompress.IsError(r)) throw new InvalidOperationException(GetErrorName(r));
            Array.Resize(ref dst, (int)r);
            return dst;
        }

        public static string GetErrorName(uint code) => Marshal.PtrToStringAnsi(zsmi_getErrorName((UIntPtr)(ulong)(long)(int)code));
    }
}
