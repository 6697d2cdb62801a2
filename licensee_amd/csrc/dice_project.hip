// Project#license on the device: the per-file results of a resident batch reduced to one record
// per project (a group of consecutive license files).
//
// Reference: lib/licensee/projects/project.rb --
//   license (:24-32)                    licenses_without_copyright.count == 1 || lgpl? -> its first entry,
//                                       more than one -> License 'other', none -> nil
//   licenses (:35-37)                   matched_files.map(&:license).uniq
//   matched_file (:40-42)               matched_files.first if matched_files.count == 1 || lgpl?
//   lgpl? (:102-106)                    two files, two licenses, files[0].lgpl? && files[1].gpl?
//   prioritize_lgpl (:137-145)          a GPL first file yields the front to the first COPYING.lesser with an LGPL license
//   licenses_without_copyright (:153-155)  the files that are not copyright? (project_file.rb:90-95)
// over LicenseFile#license (license_file.rb:92-98), which is never nil: every license file is a
// matched file. Per file i, from the flags the host gives and the resident Exact / Dice results,
//   L(i) = flags & 1 ? T + 1 : (use_exact && exact[i] >= 0) ? exact[i] : best[i] >= 0 ? best[i] : T
// (T = 'other', T + 1 = 'no-license': the Copyright matcher's license).
//
// `license` and `matched_file` do not depend on the order of a project's files: lgpl? needs exactly
// two files, one a COPYING.lesser with an LGPL license and the other with a GPL license, whichever
// comes first (prioritize_lgpl swaps them when the GPL one does); otherwise the answer is a count
// of distinct licenses. Only `licenses` is ordered (file order after prioritize_lgpl, first
// occurrence), so no sort is needed anywhere.
//
// Shape: a wave takes 64 consecutive projects. A project of at most kProjLane files is reduced by
// its own lane, which walks its contiguous segment with the licenses in registers (static indices
// only). The wave then takes its larger projects one at a time, lanes over files 64 at a time:
// ballots find the first COPYING.lesser and the first lane of every license not yet seen, and an LDS
// bitset of T + 2 bits (one per license id) carries "seen" from one 64-file step to the next, so a
// project of any size costs one pass over its files and no file-to-file compare.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "dice_common.h"
#include "dice_internal.h"

namespace dice {

constexpr int kProjLane = 8;   // files a single lane reduces; DICE_PROJECT_K_MAX licenses fit the same registers

struct ProjIn {
    const int32_t* exact;     // NULL: use_exact == 0
    const int32_t* best;
    const uint8_t* fflags;
    const uint8_t* tflags;
    int32_t T;
};

__device__ __forceinline__ int32_t proj_license(const ProjIn& in, int64_t i, uint32_t fl) {
    if (fl & 1u) return in.T + 1;
    if (in.exact) {
        const int32_t e = in.exact[i];
        if (e >= 0) return e;
    }
    const int32_t b = in.best[i];
    return b >= 0 ? b : in.T;
}

// bit 0 gpl?, bit 1 lgpl? (license.rb:200-206); 'other', 'no-license' and "no file" (-2) have neither
__device__ __forceinline__ uint32_t proj_tflags(const ProjIn& in, int32_t L) {
    return (uint32_t)L < (uint32_t)in.T ? in.tflags[L] : 0u;
}

__device__ __forceinline__ int first_lane(uint64_t bal) { return __ffsll((unsigned long long)bal) - 1; }

__global__ __launch_bounds__(kWave) void dice_project_kernel(ProjIn in, const int64_t* __restrict__ offs, int64_t P,
                                                            int32_t k, const double* __restrict__ score,
                                                            const uint32_t* __restrict__ hdig,
                                                            int32_t* __restrict__ o_lic, int32_t* __restrict__ o_mf,
                                                            int32_t* __restrict__ o_nl, int32_t* __restrict__ o_list,
                                                            int32_t* __restrict__ o_matcher, double* __restrict__ o_conf,
                                                            uint32_t* __restrict__ o_dig) {
    extern __shared__ uint32_t seen[];   // (T + 2 + 31) / 32 words: the wave path's license bitset
    const int lane = (int)threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * kWave;
    const int64_t p = p0 + lane;
    const int32_t T = in.T;
    int64_t a = 0, s = 0;
    if (p < P) {
        a = offs[p];
        s = offs[p + 1] - a;
    }
    int32_t lic = -1, mf = -1, nl = 0;

    if (p < P && s <= kProjLane) {
        // ---- one lane, one project ----
        int32_t Ls[kProjLane];
        uint32_t Fs[kProjLane];
#pragma unroll
        for (int j = 0; j < kProjLane; ++j) {
            const bool ok = j < s;
            const uint32_t fl = ok ? in.fflags[a + j] : 0u;
            Fs[j] = fl;
            Ls[j] = ok ? proj_license(in, a + j, fl) : -2;
        }
        // prioritize_lgpl: files.first.license.gpl?, then files.find_index(&:lgpl?)
        int m = -1;
#pragma unroll
        for (int j = kProjLane - 1; j >= 0; --j)
            if (j < s && (Fs[j] & 4u) && (proj_tflags(in, Ls[j]) & 2u)) m = j;
        const bool prio = (proj_tflags(in, Ls[0]) & 1u) && m > 0;
        // licenses: file order after the move, first occurrences
        int32_t Os[kProjLane];
#pragma unroll
        for (int q = 0; q < kProjLane; ++q) {
            const int idx = prio ? (q == 0 ? m : (q <= m ? q - 1 : q)) : q;
            int32_t v = -2;
#pragma unroll
            for (int r = 0; r < kProjLane; ++r) v = idx == r ? Ls[r] : v;
            Os[q] = v;
        }
#pragma unroll
        for (int q = 0; q < kProjLane; ++q) {
            bool nw = q < s;
#pragma unroll
            for (int r = 0; r < q; ++r) nw = nw && Os[r] != Os[q];
            if (nw) {
                if (nl < k) o_list[p * k + nl] = Os[q];
                ++nl;
            }
        }
        for (int j = nl; j < k; ++j) o_list[p * k + j] = -1;
        // licenses_without_copyright: distinct licenses of the files that are not copyright?
        int32_t dv = -1;
        bool multi = false;
#pragma unroll
        for (int j = 0; j < kProjLane; ++j)
            if (j < s && (Fs[j] & 3u) != 3u) {
                if (dv < 0) dv = Ls[j];
                else if (Ls[j] != dv) multi = true;
            }
        const bool lg0 = (Fs[0] & 4u) && (proj_tflags(in, Ls[0]) & 2u) && (proj_tflags(in, Ls[1]) & 1u);
        const bool lg1 = (Fs[1] & 4u) && (proj_tflags(in, Ls[1]) & 2u) && (proj_tflags(in, Ls[0]) & 1u);
        if (s == 2 && (lg0 || lg1)) {   // lgpl?: the COPYING.lesser file is first after prioritize_lgpl
            lic = lg0 ? Ls[0] : Ls[1];
            mf = (int32_t)(a + (lg0 ? 0 : 1));
        } else {
            lic = multi ? T : dv;
            mf = s == 1 ? (int32_t)a : -1;
        }
    }

    // ---- the wave's larger projects, one at a time, lanes over files ----
    uint64_t big = __ballot(p < P && s > kProjLane);
    const int words = (T + 2 + 31) >> 5;
    while (big) {
        const int src = first_lane(big);
        big &= big - 1;
        const int64_t pp = p0 + src;
        const int64_t pa = offs[pp], ps = offs[pp + 1] - pa;
        for (int w = lane; w < words; w += kWave) seen[w] = 0u;
        __syncthreads();
        const uint32_t f0 = in.fflags[pa];
        const int32_t L0 = proj_license(in, pa, f0);
        int64_t m = -1;
        if (proj_tflags(in, L0) & 1u) {
            for (int64_t base = 0; base < ps && m < 0; base += kWave) {
                const int64_t i = base + lane;
                bool ok = false;
                if (i < ps) {
                    const uint32_t fl = in.fflags[pa + i];
                    ok = (fl & 4u) && (proj_tflags(in, proj_license(in, pa + i, fl)) & 2u);
                }
                const uint64_t bal = __ballot(ok);
                if (bal) m = base + first_lane(bal);
            }
        }
        int32_t cnt = 0;
        if (m >= 0) {   // the moved file's license heads the list
            const int32_t Lm = proj_license(in, pa + m, in.fflags[pa + m]);
            if (lane == 0) {
                seen[Lm >> 5] |= 1u << (Lm & 31);
                if (k > 0) o_list[pp * k] = Lm;
            }
            cnt = 1;
            __syncthreads();
        }
        int32_t dv = -1;
        bool multi = false;
        for (int64_t base = 0; base < ps; base += kWave) {
            const int64_t i = base + lane;
            const bool valid = i < ps;
            const uint32_t fl = valid ? in.fflags[pa + i] : 0u;
            const int32_t L = valid ? proj_license(in, pa + i, fl) : 0;
            const bool nc = valid && (fl & 3u) != 3u;
            const uint64_t ncb = __ballot(nc);
            if (ncb) {
                const int32_t v = __builtin_amdgcn_readlane(L, first_lane(ncb));
                if (dv < 0) dv = v;
                if (__ballot(nc && L != dv)) multi = true;
            }
            const bool fresh = valid && !((seen[L >> 5] >> (L & 31)) & 1u);
            uint64_t rem = __ballot(fresh);
            while (rem) {   // once per license this step sees for the first time, lowest lane first
                const int32_t v = __builtin_amdgcn_readlane(L, first_lane(rem));
                rem &= ~__ballot(fresh && L == v);
                if (lane == 0) {
                    seen[v >> 5] |= 1u << (v & 31);
                    if (cnt < k) o_list[pp * k + cnt] = v;
                }
                ++cnt;
            }
            __syncthreads();
        }
        for (int j = cnt + lane; j < k; j += kWave) o_list[pp * k + j] = -1;
        if (lane == src) {   // more than two files: no lgpl?, no single matched file
            lic = multi ? T : dv;
            mf = -1;
            nl = cnt;
        }
    }

    if (p < P) {
        o_lic[p] = lic;
        o_mf[p] = mf;
        o_nl[p] = nl;
        // the matched file's matcher (0 Copyright, 1 Exact, 2 Dice, -1 none), confidence and digest
        int32_t mt = -1;
        double cf = 0.0;
        if (mf >= 0) {
            if (in.fflags[mf] & 1u) mt = 0;
            else if (in.exact && in.exact[mf] >= 0) mt = 1;
            else if (in.best[mf] >= 0) mt = 2;
            cf = mt == 2 ? score[mf] : mt >= 0 ? 100.0 : 0.0;
        }
        o_matcher[p] = mt;
        o_conf[p] = cf;
        if (hdig) {
#pragma unroll
            for (int w = 0; w < 5; ++w) o_dig[p * 5 + w] = mf >= 0 ? hdig[(int64_t)mf * 5 + w] : 0u;
        }
    }
}

}  // namespace dice

using dice::fail;

extern "C" {

int dice_batch_projects(dice_batch* b, int64_t P, const int64_t* offsets, const uint8_t* file_flags,
                        const uint8_t* template_flags, int32_t use_exact, int32_t k, void* stream) {
    if (P < 0) return fail(DICE_E_ARG, "negative n_projects");
    if (k < 0 || k > DICE_PROJECT_K_MAX) return fail(DICE_E_ARG, "k_licenses out of range");
    if (!b) return fail(DICE_E_ARG, "NULL batch");
    dice_ctx* c = b->ctx;
    const int64_t n = b->n;
    if (!offsets || !template_flags || (n > 0 && !file_flags)) return fail(DICE_E_ARG, "NULL offsets/flags");
    if (offsets[0] != 0) return fail(DICE_E_ARG, "offsets[0] must be 0");
    for (int64_t i = 0; i < P; ++i)
        if (offsets[i + 1] < offsets[i]) return fail(DICE_E_ARG, "offsets must be non-decreasing");
    if (offsets[P] != n) return fail(DICE_E_ARG, "offsets[n_projects] must equal the batch's file count");
    if (P > 0x7FFFFFFFll * dice::kWave) return fail(DICE_E_ARG, "too many projects");
    const size_t lds = (size_t)((c->T + 2 + 31) >> 5) * 4;
    if (lds > 64 * 1024) return fail(DICE_E_ARG, "too many templates for the project kernel's license bitset");
    if (b->match_epoch != b->epoch) return fail(DICE_E_STATE, "no match call has run since the last upload");
    if (use_exact && b->exact_epoch != b->epoch)
        return fail(DICE_E_STATE, "use_exact needs dice_batch_exact to have run since the last upload");
    dice::DeviceGuard g(c->device);
    hipStream_t s = dice::stream_of(c, stream);
    b->proj_epoch = 0;
    int rc;
    if (P > b->proj_cap || !b->d_poffs) {
        // (the buffers may still feed an earlier resolve or its download; proj_cap stays 0 while a
        // regrow is in flight)
        if (hipStreamSynchronize(s) != hipSuccess) return fail(DICE_E_DEVICE, "hipStreamSynchronize failed");
        const size_t cap = (size_t)std::max<int64_t>(std::max<int64_t>(P, 2 * b->proj_cap), 64);
        b->proj_cap = 0;
        if ((rc = b->d_poffs.reserve(cap + 1)) || (rc = b->d_plic.reserve(cap)) || (rc = b->d_pmf.reserve(cap)) ||
            (rc = b->d_pnl.reserve(cap)) || (rc = b->d_plist.reserve(cap * DICE_PROJECT_K_MAX)) ||
            (rc = b->d_pmatcher.reserve(cap)) || (rc = b->d_pconf.reserve(cap)) || (rc = b->d_pdig.reserve(cap * 20)))
            return rc;
        b->proj_cap = (int64_t)cap;
    }
    if ((rc = b->d_pfflags.reserve((size_t)b->capacity)) || (rc = b->d_ptflags.reserve((size_t)c->T))) return rc;
    b->proj_P = P;
    b->proj_k = k;
    b->proj_hash = b->text_state == 2;   // the digests of dice_batch_content_hash are there to gather
    if (P > 0) {
        if (hipMemcpyAsync(b->d_poffs, offsets, (size_t)(P + 1) * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
            (n && hipMemcpyAsync(b->d_pfflags, file_flags, (size_t)n, hipMemcpyHostToDevice, s) != hipSuccess) ||
            hipMemcpyAsync(b->d_ptflags, template_flags, (size_t)c->T, hipMemcpyHostToDevice, s) != hipSuccess)
            return fail(DICE_E_DEVICE, "project offsets/flags upload failed");
        dice::ProjIn in;
        in.exact = use_exact ? b->d_exact.get() : nullptr;
        in.best = b->d_best;
        in.fflags = b->d_pfflags;
        in.tflags = b->d_ptflags;
        in.T = c->T;
        const unsigned grid = (unsigned)((P + dice::kWave - 1) / dice::kWave);
        hipLaunchKernelGGL(dice::dice_project_kernel, dim3(grid), dim3(dice::kWave), lds, s, in, (const int64_t*)b->d_poffs, P,
                           k, (const double*)b->d_score, b->proj_hash ? (const uint32_t*)b->d_hdig.get() : nullptr, b->d_plic,
                           b->d_pmf, b->d_pnl, b->d_plist, b->d_pmatcher, b->d_pconf, (uint32_t*)b->d_pdig.get());
        if (hipGetLastError() != hipSuccess) return fail(DICE_E_DEVICE, "dice_project_kernel launch failed");
    }
    b->proj_epoch = b->epoch;
    return DICE_OK;
}

static int projects_ready(dice_batch* b) {
    if (!b) return fail(DICE_E_ARG, "NULL batch");
    if (b->proj_epoch != b->epoch) return fail(DICE_E_STATE, "no project resolve has run since the last upload");
    return DICE_OK;
}

int dice_batch_download_projects(dice_batch* b, int32_t* license, int32_t* matched_file, int32_t* n_licenses,
                                 int32_t* licenses, void* stream) {
    int rc = projects_ready(b);
    if (rc) return rc;
    dice_ctx* c = b->ctx;
    dice::DeviceGuard g(c->device);
    hipStream_t s = dice::stream_of(c, stream);
    const size_t P = (size_t)b->proj_P, k = (size_t)b->proj_k;
    if (P && ((license && hipMemcpyAsync(license, b->d_plic, P * 4, hipMemcpyDeviceToHost, s) != hipSuccess) ||
              (matched_file && hipMemcpyAsync(matched_file, b->d_pmf, P * 4, hipMemcpyDeviceToHost, s) != hipSuccess) ||
              (n_licenses && hipMemcpyAsync(n_licenses, b->d_pnl, P * 4, hipMemcpyDeviceToHost, s) != hipSuccess) ||
              (licenses && k && hipMemcpyAsync(licenses, b->d_plist, P * k * 4, hipMemcpyDeviceToHost, s) != hipSuccess)))
        return fail(DICE_E_DEVICE, "project download failed");
    return hipStreamSynchronize(s) == hipSuccess ? DICE_OK : fail(DICE_E_DEVICE, "hipStreamSynchronize failed");
}

int dice_batch_download_project_match(dice_batch* b, int32_t* matcher, double* confidence, uint8_t* digest, void* stream) {
    int rc = projects_ready(b);
    if (rc) return rc;
    if (digest && !b->proj_hash)
        return fail(DICE_E_STATE, "no content hash was computed before the project resolve");
    dice_ctx* c = b->ctx;
    dice::DeviceGuard g(c->device);
    hipStream_t s = dice::stream_of(c, stream);
    const size_t P = (size_t)b->proj_P;
    if (P && ((matcher && hipMemcpyAsync(matcher, b->d_pmatcher, P * 4, hipMemcpyDeviceToHost, s) != hipSuccess) ||
              (confidence && hipMemcpyAsync(confidence, b->d_pconf, P * 8, hipMemcpyDeviceToHost, s) != hipSuccess) ||
              (digest && hipMemcpyAsync(digest, b->d_pdig, P * 20, hipMemcpyDeviceToHost, s) != hipSuccess)))
        return fail(DICE_E_DEVICE, "project match download failed");
    return hipStreamSynchronize(s) == hipSuccess ? DICE_OK : fail(DICE_E_DEVICE, "hipStreamSynchronize failed");
}

}  // extern "C"
