// ContentHelper#content_hash on the device: SHA-1 of every resident normalized text.
//
// Reference: lib/licensee/content_helper.rb:136-138 --
//   def content_hash; @content_hash ||= DIGEST.hexdigest content_normalized; end   (DIGEST = Digest::SHA1)
// one of ProjectFile's HASH_METHODS (project_file.rb:17,97) and a field of `licensee detect`.
//
// The texts are those an upload left in HBM (dice_words.hip: 16-byte aligned offsets, 64 bytes of
// slack past the texts). After dice_batch_upload_text_utf8 they are the UTF-8 of content_normalized,
// so their SHA-1 is content_hash and no file is flagged. After dice_batch_upload_text they hold one
// byte per character, every non-ASCII character as 0x80: an ASCII text's digest is content_hash, a
// text with a byte >= 0x80 is flagged (status 1) and its digest is that of the resident bytes. The
// flag is (OR of the file's bytes) & flag_mask: 0x80808080 for the one-byte form, 0 for UTF-8.
//
// SHA-1 is one serial chain per message, so the parallelism is across files: one lane per file,
// persistent. Every loop iteration each live lane runs one 64-byte block; a lane that finishes its
// file stores the digest and takes the next file index from a device counter, so a short file next
// to a long one does not idle its lane, and a lane leaves when the counter has passed n. A block
// is four aligned 16-byte loads, requested one block ahead of the 80 rounds that use them; a
// 16-byte group is loaded only when it starts inside the file, so no load leaves the allocation
// even when the last file ends exactly at text_bytes. Bytes at or past the file's length (another
// file's padding, uninitialised slack) are masked, never trusted: a block that reaches the end of
// the text takes the padding path (mask, 0x80, the bit length in words 14-15 of the last block).
// The 16-word schedule rolls in registers with static indices only; Ch, Parity, Maj and the
// schedule's xor are v_bitop3_b32, the rotates v_alignbit_b32, the sums v_add3_u32.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dice_common.h"
#include "dice_internal.h"

namespace dice {

__device__ __forceinline__ uint32_t rotl(uint32_t x, uint32_t n) { return __builtin_amdgcn_alignbit(x, x, 32u - n); }
// A boolean function of three words in one instruction (v_bitop3_b32): result bit = bit (4a + 2b + c)
// of the truth table TT, i.e. TT is the function applied to 0xF0, 0xCC, 0xAA. gfx950 has no
// three-input xor, and the compiler left to itself spends two instructions on each of these.
template <int TT>
__device__ __forceinline__ uint32_t bitop3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, TT);
}
constexpr int kCh = 0xCA, kParity = 0x96, kMaj = 0xE8;   // (a & b) | (~a & c);  a ^ b ^ c;  majority

struct Sha1Block {
    uint4 q[4];
};

// the 16-byte groups of the block at byte `pos` that start inside the file (the others stay zero)
__device__ __forceinline__ void sha1_request(Sha1Block& b, const uint4* __restrict__ p, uint32_t pos, uint32_t len) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        b.q[g] = make_uint4(0u, 0u, 0u, 0u);
        if (pos + 16u * g < len) b.q[g] = p[(pos >> 4) + g];
    }
}

__global__ __launch_bounds__(kWave) void dice_sha1_kernel(const uint8_t* __restrict__ text,
                                                          const int64_t* __restrict__ toff,
                                                          const int32_t* __restrict__ tlen, int64_t n,
                                                          uint32_t* __restrict__ next, uint32_t* __restrict__ digest,
                                                          uint8_t* __restrict__ status, uint32_t flag_mask) {
    int64_t f = atomicAdd(next, 1u);
    if (f >= n) return;
    const uint4* p = reinterpret_cast<const uint4*>(text + toff[f]);
    uint32_t len = (uint32_t)tlen[f];
    uint32_t pos = 0, end = ((len + 8u) / 64u + 1u) * 64u;   // len < 2^31: no wrap
    uint32_t h0 = 0x67452301u, h1 = 0xEFCDAB89u, h2 = 0x98BADCFEu, h3 = 0x10325476u, h4 = 0xC3D2E1F0u;
    uint32_t seen = 0;   // OR of the file's in-range bytes
    Sha1Block nb;
    sha1_request(nb, p, 0u, len);
    for (;;) {
        uint32_t w[16] = {nb.q[0].x, nb.q[0].y, nb.q[0].z, nb.q[0].w, nb.q[1].x, nb.q[1].y, nb.q[1].z, nb.q[1].w,
                          nb.q[2].x, nb.q[2].y, nb.q[2].z, nb.q[2].w, nb.q[3].x, nb.q[3].y, nb.q[3].z, nb.q[3].w};
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = __builtin_bswap32(w[i]);
        // the next block's loads, in flight over this block's rounds (none past the file's end);
        // requested after the swaps have consumed this block's, so that the wait for these (their
        // number depends on the lane) comes only with the next block's swaps. The empty statement
        // pins the swaps here: the compiler otherwise sinks them below the loads.
        asm volatile("" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]), "+v"(w[6]), "+v"(w[7]),
                          "+v"(w[8]), "+v"(w[9]), "+v"(w[10]), "+v"(w[11]), "+v"(w[12]), "+v"(w[13]), "+v"(w[14]),
                          "+v"(w[15]));
        sha1_request(nb, p, pos + 64u, len);
        const int32_t t = (int32_t)(len - pos);   // bytes of the file from this block on (<= 0: padding only)
        if (t < 64) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int32_t r = t - 4 * i;      // in-range bytes from word i on
                const uint32_t k = (uint32_t)(r < 0 ? 0 : r > 4 ? 4 : r);
                w[i] &= (uint32_t)(0xFFFFFFFF00000000ull >> (8u * k));
                seen |= w[i];
                if ((uint32_t)r < 4u) w[i] |= 0x80000000u >> (8u * (uint32_t)r);
            }
            if (pos + 64u == end) {
                w[14] = len >> 29;
                w[15] = len << 3;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) seen |= w[i];
        }
        uint32_t a = h0, b = h1, c = h2, d = h3, e = h4;
#pragma unroll
        for (int i = 0; i < 80; ++i) {
            if (i >= 16) w[i & 15] = rotl(bitop3<kParity>(w[(i + 13) & 15], w[(i + 8) & 15], w[(i + 2) & 15]) ^ w[i & 15], 1);
            uint32_t fn, kc;
            if (i < 20) {
                fn = bitop3<kCh>(b, c, d);
                kc = 0x5A827999u;
            } else if (i < 40) {
                fn = bitop3<kParity>(b, c, d);
                kc = 0x6ED9EBA1u;
            } else if (i < 60) {
                fn = bitop3<kMaj>(b, c, d);
                kc = 0x8F1BBCDCu;
            } else {
                fn = bitop3<kParity>(b, c, d);
                kc = 0xCA62C1D6u;
            }
            const uint32_t tmp = rotl(a, 5) + fn + (e + kc + w[i & 15]);
            e = d;
            d = c;
            c = rotl(b, 30);
            b = a;
            a = tmp;
        }
        h0 += a;
        h1 += b;
        h2 += c;
        h3 += d;
        h4 += e;
        pos += 64u;
        if (pos == end) {
            uint32_t* o = digest + f * 5;
            o[0] = __builtin_bswap32(h0);
            o[1] = __builtin_bswap32(h1);
            o[2] = __builtin_bswap32(h2);
            o[3] = __builtin_bswap32(h3);
            o[4] = __builtin_bswap32(h4);
            status[f] = (seen & flag_mask) ? 1 : 0;
            f = atomicAdd(next, 1u);
            if (f >= n) break;
            p = reinterpret_cast<const uint4*>(text + toff[f]);
            len = (uint32_t)tlen[f];
            pos = 0;
            end = ((len + 8u) / 64u + 1u) * 64u;
            h0 = 0x67452301u, h1 = 0xEFCDAB89u, h2 = 0x98BADCFEu, h3 = 0x10325476u, h4 = 0xC3D2E1F0u;
            seen = 0;
            sha1_request(nb, p, 0u, len);
        }
    }
}

}  // namespace dice

using dice::fail;

extern "C" {

int dice_batch_content_hash(dice_batch* b, void* stream) {
    if (!b) return fail(DICE_E_ARG, "NULL batch");
    dice_ctx* c = b->ctx;
    if (!b->text_state)
        return fail(DICE_E_STATE, "the batch's last upload was not dice_batch_upload_text or dice_batch_upload_text_utf8");
    const int64_t n = b->n;
    if (n == 0) {
        b->text_state = 2;
        return DICE_OK;
    }
    dice::DeviceGuard g(c->device);
    hipStream_t s = dice::stream_of(c, stream);
    int rc;
    // digests [capacity][20] (read as 5 words each), status [capacity], the file counter
    if ((rc = b->d_hdig.reserve((size_t)b->capacity * 20)) || (rc = b->d_hstat.reserve((size_t)b->capacity)) ||
        (rc = b->d_hcnt.reserve(1)))
        return rc;
    if (hipMemsetAsync(b->d_hcnt, 0, 4, s) != hipSuccess) return fail(DICE_E_DEVICE, "hipMemsetAsync failed");
    // one lane per file; at most 16 waves per SIMD's worth of lanes, the rest of the files are
    // taken from the counter
    const int64_t waves = std::min<int64_t>((n + dice::kWave - 1) / dice::kWave, (int64_t)c->n_cu * 16);
    hipLaunchKernelGGL(dice::dice_sha1_kernel, dim3((unsigned)waves), dim3(dice::kWave), 0, s, (const uint8_t*)b->d_text,
                       (const int64_t*)b->d_toff, (const int32_t*)b->d_tlen, n, b->d_hcnt, (uint32_t*)b->d_hdig.get(), b->d_hstat,
                       b->text_utf8 ? 0u : 0x80808080u);
    if (hipGetLastError() != hipSuccess) return fail(DICE_E_DEVICE, "dice_sha1_kernel launch failed");
    b->text_state = 2;
    return DICE_OK;
}

int dice_batch_download_content_hash(dice_batch* b, uint8_t* digest, uint8_t* status, void* stream) {
    if (!b) return fail(DICE_E_ARG, "NULL batch");
    dice_ctx* c = b->ctx;
    if (b->text_state != 2) return fail(DICE_E_STATE, "no content hash was computed since the last upload");
    dice::DeviceGuard g(c->device);
    hipStream_t s = dice::stream_of(c, stream);
    const size_t n = (size_t)b->n;
    if (n && ((digest && hipMemcpyAsync(digest, b->d_hdig, n * 20, hipMemcpyDeviceToHost, s) != hipSuccess) ||
              (status && hipMemcpyAsync(status, b->d_hstat, n, hipMemcpyDeviceToHost, s) != hipSuccess)))
        return fail(DICE_E_DEVICE, "content hash download failed");
    return hipStreamSynchronize(s) == hipSuccess ? DICE_OK : fail(DICE_E_DEVICE, "hipStreamSynchronize failed");
}

}  // extern "C"
