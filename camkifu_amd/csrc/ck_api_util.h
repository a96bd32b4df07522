// ck_api_util.h -- what the translation units of the entry points share (ck_api.hip, ck_api_jpeg.hip, ck_api_png.hip)
#pragma once
#include "ck_common.h"

// The mirror of ck_to_device for a result of `bytes` that the caller wants at `user`: open() gives the device pointer the
// kernels write -- `user` itself, or `stage` when the caller's memory is the host's -- and deliver() then copies it home.
// A space other than CK_HOST is taken for device memory, unchecked, as it always was.  A NULL `user` stays NULL.
template <class T>
struct OutStage {
    T* dev = nullptr;
    T* user = nullptr;
    size_t bytes = 0;
    int open(ck_ctx* ctx, T* user_ptr, size_t nbytes, int space, DevBuf& stage)
    {
        dev = user_ptr;
        if (!user_ptr || space != CK_HOST) return CK_OK;
        CK_TRY(ck_ensure(ctx, stage, nbytes));
        dev = (T*)stage.p; user = user_ptr; bytes = nbytes;
        return CK_OK;
    }
    int deliver(ck_ctx* ctx) const { return user ? ck_from_device(ctx, user, dev, bytes, CK_HOST) : CK_OK; }
};

// the end of an entry point: the stream idle, and nothing failed on it
static inline int finish(ck_ctx* ctx)
{
    CK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    CK_HIP(ctx, hipGetLastError());
    return CK_OK;
}

// the two alignment refusals of the JPEG calls (include/camkifu_amd.h, "Alignment of device memory"), worded once (ck_api.hip)
int ck_coef_on_16(ck_ctx* ctx, const void* coef);
int ck_coef_quant_on_16(ck_ctx* ctx, const void* coef, const void* quant);

// The bracket of an entry point that takes no context: nothing thrown across the C ABI (CK_API_BEGIN / CK_API_END are the
// pair for the others); the message is read with ck_last_error(NULL).
#define CK_HOST_BEGIN try {
#define CK_HOST_END                                                                                       \
    } catch (const std::exception& e__) {                                                                 \
        return ck_fail(nullptr, CK_ERR_STATE, "C++ exception inside the library: %s", e__.what());        \
    }
