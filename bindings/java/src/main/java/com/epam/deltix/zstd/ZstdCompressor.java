// UNVERIFIED (no JDK in the build image).  The compressor the reference's Java side lacks, in the shape of its ZstdDecompressor: one frame per
// call, made on the GPU through the JNI shim bindings/java/jni/zsmi_jni.c over libzsmi.so (include/zsmi.h: zsmi_compress_advanced).
package com.epam.deltix.zstd;

public class ZstdCompressor {
    static {
        System.loadLibrary("zsmi_jni");
    }

    public static final int DEFAULT_LEVEL = 3;

    // result >= 0: bytes written; < 0: -(error code of csharp/src/ZStdErrors.cs:61-90)
    private static native long nCompress(byte[] input, int inputOffset, int inputLength, byte[] output, int outputOffset, int maxOutputLength, int level, boolean checksum);

    public int compress(final byte[] input, final int inputOffset, final int inputLength,
                        final byte[] output, final int outputOffset, final int maxOutputLength) {
        return compress(input, inputOffset, inputLength, output, outputOffset, maxOutputLength, DEFAULT_LEVEL, false);
    }

    // checksum: the frame carries a Content_Checksum (ZSTD_c_checksumFlag) - the same frame otherwise, 4 bytes longer; ZstdDecompressor
    // (every zstd decoder) then throws "Restored data doesn't match checksum" for a frame whose content it cannot restore
    public int compress(final byte[] input, final int inputOffset, final int inputLength,
                        final byte[] output, final int outputOffset, final int maxOutputLength, final int level, final boolean checksum) {
        checkRange(input, inputOffset, inputLength);
        checkRange(output, outputOffset, maxOutputLength);
        final long r = nCompress(input, inputOffset, inputLength, output, outputOffset, maxOutputLength, level, checksum);
        if (r < 0)
            throw new RuntimeException("compress: error " + (-r) + ": offset=" + inputOffset);
        return (int) r;
    }

    private static void checkRange(final byte[] a, final int off, final int len) {
        if (a == null) throw new NullPointerException();
        if (off < 0 || len < 0 || off > a.length - len) throw new IndexOutOfBoundsException("offset=" + off + " length=" + len + " array=" + a.length);
    }
}
