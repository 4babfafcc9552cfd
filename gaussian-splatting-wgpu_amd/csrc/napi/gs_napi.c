/*
 * gs_napi.c -- plain-C N-API shim over include/gsplat/gs_abi.h (NAPI v4+, Node >= 12).
 *
 * This is the binding a Node host uses to put the MI355X rasterizer behind the reference's
 * TypeScript surface (Renderer / Camera / PackedGaussians, see ../../js).  It adds nothing to the
 * C ABI: every export is a 1:1 wrapper; HIP errors become thrown JS Errors / rejected Promises.
 * The per-frame call never blocks the JS thread: renderAsync() enqueues and waits in a libuv worker
 * (napi_async_work) and resolves a Promise, which is what Renderer.animate() awaits where the
 * reference awaits queue.onSubmittedWorkDone() (renderer.ts:404-587).
 */
#define NAPI_VERSION 4
#include <node_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../../include/gsplat/gs_abi.h"

#define NAPI_CALL(env, call)                                              \
    do {                                                                  \
        napi_status s_ = (call);                                          \
        if (s_ != napi_ok) {                                              \
            napi_throw_error((env), NULL, "N-API call failed: " #call);   \
            return NULL;                                                  \
        }                                                                 \
    } while (0)

static napi_value throw_gs(napi_env env, int32_t rc) {
    char msg[640];
    const char* e = gs_last_error();
    strcpy(msg, "gsplat: ");
    strncat(msg, e && e[0] ? e : "error", sizeof(msg) - 32);
    char code[16];
    int n = 0, v = rc < 0 ? -rc : rc;
    code[n++] = '-';
    if (v >= 10) code[n++] = (char)('0' + v / 10);
    code[n++] = (char)('0' + v % 10);
    code[n] = 0;
    napi_throw_error(env, code, msg);
    return NULL;
}

static int get_u32_prop(napi_env env, napi_value obj, const char* name, uint32_t* out) {
    napi_value v;
    bool has = false;
    if (napi_has_named_property(env, obj, name, &has) != napi_ok || !has) return 0;
    if (napi_get_named_property(env, obj, name, &v) != napi_ok) return 0;
    double d;
    if (napi_get_value_double(env, v, &d) != napi_ok) return 0;
    *out = (uint32_t)d;
    return 1;
}

static void set_num(napi_env env, napi_value obj, const char* k, double v) {
    napi_value n;
    napi_create_double(env, v, &n);
    napi_set_named_property(env, obj, k, n);
}

/* what a wrapper of a call that reports nothing returns: throws on rc */
static napi_value ret_none(napi_env env, int32_t rc) { return rc == GS_OK ? NULL : throw_gs(env, rc); }
/* what a wrapper of a call that reports a count returns: throws on rc, otherwise the value as a double */
static napi_value ret_u64(napi_env env, int32_t rc, uint64_t value) {
    if (rc != GS_OK) return throw_gs(env, rc);
    napi_value out;
    NAPI_CALL(env, napi_create_double(env, (double)value, &out));
    return out;
}

/* The external holds a box so that destroy() can null the context.  A gs_ctx is not re-entrant and renderAsync() works on it
 * from a libuv worker: while a frame is in flight (`busy`) every other call on the handle is refused, and destroy() is
 * deferred to the frame's completion (all of this happens on the JS thread, so the flags need no lock). */
typedef struct {
    gs_ctx* ctx;
    int busy;            /* a renderAsync job owns the context */
    int inflight;        /* renderToSink frames whose tickets are being waited for on workers (they only call gs_wait_ticket) */
    int destroy_pending; /* destroy() was called meanwhile */
} ctx_box;

static ctx_box* unbox(napi_env env, napi_value v) {
    void* p = NULL;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p) {
        napi_throw_type_error(env, NULL, "gsplat: expected a context handle");
        return NULL;
    }
    return (ctx_box*)p;
}

static gs_ctx* unwrap(napi_env env, napi_value v) {
    ctx_box* b = unbox(env, v);
    if (!b) return NULL;
    if (!b->ctx) {
        napi_throw_error(env, NULL, "gsplat: the context has been destroyed");
        return NULL;
    }
    if (b->busy || b->inflight) {
        napi_throw_error(env, NULL, "gsplat: a frame is in flight on this context (await renderAsync / the renderToSink promises first)");
        return NULL;
    }
    return b->ctx;
}

static void finalize_ctx(napi_env env, void* data, void* hint) {
    (void)env; (void)hint;
    ctx_box* box = (ctx_box*)data;
    if (box->busy || box->inflight) { box->destroy_pending = 2; return; } /* the last job frees the box when it completes */
    if (box->ctx) gs_destroy(box->ctx);
    free(box);
}

/* bytes of an ArrayBuffer or of any TypedArray/Buffer view */
static int get_bytes(napi_env env, napi_value v, void** data, size_t* len) {
    bool is = false;
    if (napi_is_arraybuffer(env, v, &is) == napi_ok && is) return napi_get_arraybuffer_info(env, v, data, len) == napi_ok;
    if (napi_is_typedarray(env, v, &is) == napi_ok && is) {
        napi_typedarray_type t;
        size_t n, off;
        napi_value ab;
        if (napi_get_typedarray_info(env, v, &t, &n, data, &ab, &off) != napi_ok) return 0;
        static const size_t sz[] = {1, 1, 1, 2, 2, 4, 4, 4, 8, 8, 8};
        *len = n * sz[t];
        return 1;
    }
    if (napi_is_buffer(env, v, &is) == napi_ok && is) return napi_get_buffer_info(env, v, data, len) == napi_ok;
    return 0;
}

/* Every wrapper's prologue.  ARGS(max): argc and argv[max].  CTX_ARGS(max, need) also yields the unwrapped context of argv[0] in
 * `ctx`, or returns: undefined for a call with fewer than `need` arguments, with unwrap's exception pending otherwise. */
#define ARGS(max)         \
    size_t argc = (max);  \
    napi_value argv[max]; \
    NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL))
#define CTX_ARGS(max, need)                                     \
    ARGS(max);                                                  \
    gs_ctx* ctx = argc >= (need) ? unwrap(env, argv[0]) : NULL; \
    if (!ctx) return NULL

/* The size protocol of the C ABI as an ArrayBuffer: ask for the count (dst NULL), create count * elem bytes, call again to fill.
 * a: the call's own arguments. */
typedef int32_t (*fill_fn)(gs_ctx* ctx, const uint32_t* a, void* dst, uint64_t cap, uint64_t* n);
static napi_value fill_arraybuffer(napi_env env, gs_ctx* ctx, fill_fn fn, const uint32_t* a, size_t elem) {
    uint64_t n = 0;
    int32_t rc = fn(ctx, a, NULL, 0, &n);
    if (rc != GS_OK) return throw_gs(env, rc);
    void* dst = NULL;
    napi_value ab;
    NAPI_CALL(env, napi_create_arraybuffer(env, (size_t)n * elem, &dst, &ab));
    if (n) rc = fn(ctx, a, dst, n, &n);
    return rc == GS_OK ? ab : throw_gs(env, rc);
}
static int32_t fill_buffer(gs_ctx* ctx, const uint32_t* a, void* dst, uint64_t cap, uint64_t* n) { /* a[0]: GS_BUF_*; bytes */
    return gs_read_buffer(ctx, (int32_t)a[0], dst, cap, n);
}
static int32_t fill_coverage(gs_ctx* ctx, const uint32_t* a, void* dst, uint64_t cap, uint64_t* n) {
    (void)a;
    return gs_coverage_read(ctx, (gs_coverage_rec*)dst, cap, n);
}
static int32_t fill_list(gs_ctx* ctx, const uint32_t* a, void* dst, uint64_t cap, uint64_t* n) { /* a: mask, value */
    return gs_state_list(ctx, a[0], a[1], (uint32_t*)dst, cap, n);
}

/* obj.mask (bytes) with obj.maskWidth and obj.maskHeight: the mask covers the CANVAS (the JS Renderer passes its canvas size),
 * checked against the bytes given.  *mask stays as it is without a usable obj.mask.  Returns 0 with a TypeError pending. */
static int get_mask_prop(napi_env env, napi_value obj, const char* who, const uint8_t** mask) {
    napi_value v;
    bool has = false;
    void* data = NULL;
    size_t len = 0;
    if (napi_has_named_property(env, obj, "mask", &has) != napi_ok || !has || napi_get_named_property(env, obj, "mask", &v) != napi_ok ||
        !get_bytes(env, v, &data, &len))
        return 1;
    uint32_t cw = 0, ch = 0;
    if (!get_u32_prop(env, obj, "maskWidth", &cw) || !get_u32_prop(env, obj, "maskHeight", &ch) || (double)len < (double)cw * (double)ch) {
        char msg[128];
        snprintf(msg, sizeof(msg), "gsplat.%s: mask needs maskWidth, maskHeight and width * height bytes", who);
        napi_throw_type_error(env, NULL, msg);
        return 0;
    }
    *mask = (const uint8_t*)data;
    return 1;
}

/* create({width,height,tileSize,device,colBegin,colEnd,flags,maxIntersections}) -> handle */
static napi_value js_create(napi_env env, napi_callback_info info) {
    ARGS(1);
    gs_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.struct_size = sizeof(cfg);
    cfg.tile_size = 16;
    uint32_t dev = 0, maxi = 0;
    if (argc < 1 || !get_u32_prop(env, argv[0], "width", &cfg.width) || !get_u32_prop(env, argv[0], "height", &cfg.height)) {
        napi_throw_type_error(env, NULL, "gsplat.create: {width, height} required");
        return NULL;
    }
    get_u32_prop(env, argv[0], "tileSize", &cfg.tile_size);
    if (get_u32_prop(env, argv[0], "device", &dev)) cfg.device = (int32_t)dev;
    get_u32_prop(env, argv[0], "colBegin", &cfg.col_begin);
    get_u32_prop(env, argv[0], "colEnd", &cfg.col_end);
    get_u32_prop(env, argv[0], "flags", &cfg.flags);
    if (get_u32_prop(env, argv[0], "maxIntersections", &maxi)) cfg.max_intersections = maxi;
    gs_ctx* ctx = NULL;
    int32_t rc = gs_create(&cfg, &ctx);
    if (rc != GS_OK) return throw_gs(env, rc);
    ctx_box* box = (ctx_box*)calloc(1, sizeof(ctx_box));
    if (!box) { gs_destroy(ctx); napi_throw_error(env, NULL, "gsplat.create: out of memory"); return NULL; }
    box->ctx = ctx;
    napi_value ext;
    if (napi_create_external(env, box, finalize_ctx, NULL, &ext) != napi_ok) {
        gs_destroy(ctx);
        free(box);
        napi_throw_error(env, NULL, "N-API call failed: napi_create_external");
        return NULL;
    }
    return ext;
}

static napi_value js_destroy(napi_env env, napi_callback_info info) {
    ARGS(1);
    void* p = NULL;
    if (argc < 1 || napi_get_value_external(env, argv[0], &p) != napi_ok || !p) return NULL;
    ctx_box* box = (ctx_box*)p;
    if (box->busy || box->inflight) { /* a frame is in flight on a worker: destroy when it completes */
        if (!box->destroy_pending) box->destroy_pending = 1;
        return NULL;
    }
    if (box->ctx) {
        gs_destroy(box->ctx);
        box->ctx = NULL;
    }
    return NULL;
}

/* uploadSplats(handle, bytes, n) */
static napi_value js_upload(napi_env env, napi_callback_info info) {
    CTX_ARGS(3, 3);
    void* data = NULL;
    size_t len = 0;
    double n = 0;
    if (!get_bytes(env, argv[1], &data, &len) || napi_get_value_double(env, argv[2], &n) != napi_ok || !(n >= 0.0) ||
        n != (double)(uint64_t)n || n >= 2147483648.0 || (double)len < n * GS_SPLAT_RECORD_BYTES) {
        napi_throw_type_error(env, NULL, "gsplat.uploadSplats: need n*320 bytes");
        return NULL;
    }
    return ret_none(env, gs_upload_splats(ctx, data, (uint64_t)n));
}

/* shareSplats(handle, ownerHandle): render the owner's resident splats from a second context (gs_share_splats) */
static napi_value js_share(napi_env env, napi_callback_info info) {
    CTX_ARGS(2, 2);
    gs_ctx* owner = unwrap(env, argv[1]);
    if (!owner) return NULL;
    return ret_none(env, gs_share_splats(ctx, owner));
}

/* renderSync(handle, uniforms160[, debug]) : enqueue + wait on the calling thread */
static napi_value js_render_sync(napi_env env, napi_callback_info info) {
    CTX_ARGS(3, 2);
    void* data = NULL;
    size_t len = 0;
    if (!get_bytes(env, argv[1], &data, &len) || len < GS_UNIFORM_BYTES) {
        napi_throw_type_error(env, NULL, "gsplat.render: need the 160-byte uniform block");
        return NULL;
    }
    bool debug = false;
    if (argc >= 3) napi_get_value_bool(env, argv[2], &debug);
    int32_t rc = debug ? gs_render_debug(ctx, data) : gs_render(ctx, data);
    if (rc == GS_OK) rc = gs_wait(ctx);
    return rc == GS_OK ? NULL : throw_gs(env, rc);
}

typedef struct {
    napi_async_work work;
    napi_deferred deferred;
    ctx_box* box;
    gs_ctx* ctx;
    unsigned char uniforms[GS_UNIFORM_BYTES];
    int32_t rc;
    char err[512];
} frame_job;

static void job_execute(napi_env env, void* data) {
    (void)env;
    frame_job* j = (frame_job*)data;
    j->rc = gs_render(j->ctx, j->uniforms);
    if (j->rc == GS_OK) j->rc = gs_wait(j->ctx);
    if (j->rc != GS_OK) { /* gs_last_error is thread-local: capture it on the worker thread */
        strncpy(j->err, gs_last_error(), sizeof(j->err) - 1);
        j->err[sizeof(j->err) - 1] = 0;
    }
}

/* What the completion of a renderAsync or renderToSink job does once the job has given the context back (busy = 0, inflight--):
 * the destroy() (1) or the finalizer (2) that came while frames were in flight, then the promise. */
static void finish_job(napi_env env, ctx_box* box, napi_deferred deferred, napi_status status, int32_t rc, const char* err) {
    napi_value v;
    if (!box->inflight && !box->busy && box->destroy_pending) {
        if (box->ctx) gs_destroy(box->ctx);
        box->ctx = NULL;
        if (box->destroy_pending == 2) free(box);
        else box->destroy_pending = 0;
    }
    if (status == napi_ok && rc == GS_OK) {
        napi_get_undefined(env, &v);
        napi_resolve_deferred(env, deferred, v);
    } else {
        napi_value msg;
        napi_create_string_utf8(env, rc != GS_OK ? err : "gsplat: async work cancelled", NAPI_AUTO_LENGTH, &msg);
        napi_create_error(env, NULL, msg, &v);
        napi_reject_deferred(env, deferred, v);
    }
}

static void job_complete(napi_env env, napi_status status, void* data) {
    frame_job* j = (frame_job*)data;
    j->box->busy = 0; /* (no renderToSink frame is in flight beside a renderAsync job: each refuses the other) */
    finish_job(env, j->box, j->deferred, status, j->rc, j->err);
    napi_delete_async_work(env, j->work);
    free(j);
}

/* renderAsync(handle, uniforms160) -> Promise<void> */
static napi_value js_render_async(napi_env env, napi_callback_info info) {
    CTX_ARGS(2, 2);
    void* data = NULL;
    size_t len = 0;
    if (!get_bytes(env, argv[1], &data, &len) || len < GS_UNIFORM_BYTES) {
        napi_throw_type_error(env, NULL, "gsplat.renderAsync: need the 160-byte uniform block");
        return NULL;
    }
    frame_job* j = (frame_job*)calloc(1, sizeof(frame_job));
    if (!j) { napi_throw_error(env, NULL, "gsplat.renderAsync: out of memory"); return NULL; }
    j->box = unbox(env, argv[0]);
    j->ctx = ctx;
    memcpy(j->uniforms, data, GS_UNIFORM_BYTES);
    napi_value promise, name;
    if (napi_create_promise(env, &j->deferred, &promise) != napi_ok ||
        napi_create_string_utf8(env, "gsplat.frame", NAPI_AUTO_LENGTH, &name) != napi_ok ||
        napi_create_async_work(env, NULL, name, job_execute, job_complete, j, &j->work) != napi_ok) {
        free(j);
        napi_throw_error(env, NULL, "gsplat.renderAsync: N-API call failed");
        return NULL;
    }
    j->box->busy = 1;
    if (napi_queue_async_work(env, j->work) != napi_ok) {
        j->box->busy = 0;
        napi_delete_async_work(env, j->work);
        free(j);
        napi_throw_error(env, NULL, "gsplat.renderAsync: napi_queue_async_work failed");
        return NULL;
    }
    return promise;
}

/* readRgba8(handle) -> ArrayBuffer (height*slabWidth*4) */
static napi_value js_read_rgba8(napi_env env, napi_callback_info info) {
    CTX_ARGS(1, 1);
    const uint32_t which = GS_BUF_RGBA8;
    return fill_arraybuffer(env, ctx, fill_buffer, &which, 1);
}

/* readBuffer(handle, which) -> ArrayBuffer */
static napi_value js_read_buffer(napi_env env, napi_callback_info info) {
    CTX_ARGS(2, 2);
    int32_t which = 0;
    NAPI_CALL(env, napi_get_value_int32(env, argv[1], &which));
    const uint32_t a = (uint32_t)which;
    return fill_arraybuffer(env, ctx, fill_buffer, &a, 1);
}

/* pick(handle, queries ( Uint32Array x,y pairs ), maxContrib) -> {results: ArrayBuffer (48 bytes per query), contrib: ArrayBuffer | null} */
static napi_value js_pick(napi_env env, napi_callback_info info) {
    CTX_ARGS(3, 2);
    void* q = NULL;
    size_t qlen = 0;
    if (!get_bytes(env, argv[1], &q, &qlen) || qlen % sizeof(gs_pick_query) != 0) {
        napi_throw_type_error(env, NULL, "gsplat: pick expects a Uint32Array of x,y pairs");
        return NULL;
    }
    uint32_t max_contrib = 0;
    if (argc >= 3) NAPI_CALL(env, napi_get_value_uint32(env, argv[2], &max_contrib));
    const size_t n = qlen / sizeof(gs_pick_query);
    if (n == 0 || n > GS_PICK_MAX_QUERIES || max_contrib > GS_PICK_MAX_CONTRIB) { /* (they size the buffers below) */
        napi_throw_range_error(env, NULL, "gsplat: pick takes 1..65536 queries and maxContrib 0..256");
        return NULL;
    }
    void *res = NULL, *con = NULL;
    napi_value res_ab, con_ab, out;
    NAPI_CALL(env, napi_create_arraybuffer(env, n * sizeof(gs_pick_result), &res, &res_ab));
    if (max_contrib) NAPI_CALL(env, napi_create_arraybuffer(env, n * max_contrib * sizeof(gs_pick_contrib), &con, &con_ab));
    else NAPI_CALL(env, napi_get_null(env, &con_ab));
    int32_t rc = gs_pick(ctx, (const gs_pick_query*)q, (uint32_t)n, (gs_pick_result*)res, max_contrib, (gs_pick_contrib*)con);
    if (rc != GS_OK) return throw_gs(env, rc);
    NAPI_CALL(env, napi_create_object(env, &out));
    NAPI_CALL(env, napi_set_named_property(env, out, "results", res_ab));
    NAPI_CALL(env, napi_set_named_property(env, out, "contrib", con_ab));
    return out;
}

/* ---- coverage: 1:1 wrappers of gs_coverage_* and gs_state_coverage ---------------------------------------------------------- */
/* accumulateCoverage(handle, region | null) -> pixels; region = {x0, y0, x1, y1, mask, maskWidth, maskHeight} (canvas pixels) */
static napi_value js_coverage_accumulate(napi_env env, napi_callback_info info) {
    CTX_ARGS(2, 1);
    gs_cover_region rg;
    memset(&rg, 0, sizeof(rg));
    rg.struct_size = sizeof(rg);
    napi_valuetype t = napi_undefined;
    if (argc >= 2) NAPI_CALL(env, napi_typeof(env, argv[1], &t));
    const int have = t == napi_object;
    if (have) {
        if (!get_u32_prop(env, argv[1], "x0", &rg.x0) || !get_u32_prop(env, argv[1], "y0", &rg.y0) || !get_u32_prop(env, argv[1], "x1", &rg.x1) ||
            !get_u32_prop(env, argv[1], "y1", &rg.y1)) {
            napi_throw_type_error(env, NULL, "gsplat.accumulateCoverage: {x0, y0, x1, y1} required");
            return NULL;
        }
        if (!get_mask_prop(env, argv[1], "accumulateCoverage", &rg.mask)) return NULL;
    }
    uint64_t pixels = 0;
    int32_t rc = gs_coverage_accumulate(ctx, have ? &rg : NULL, &pixels);
    return ret_u64(env, rc, pixels);
}

/* resetCoverage(handle) */
static napi_value js_coverage_reset(napi_env env, napi_callback_info info) {
    CTX_ARGS(1, 1);
    return ret_none(env, gs_coverage_reset(ctx));
}

/* readCoverage(handle) -> ArrayBuffer (N records of 16 bytes: gs_coverage_rec) */
static napi_value js_coverage_read(napi_env env, napi_callback_info info) {
    CTX_ARGS(1, 1);
    return fill_arraybuffer(env, ctx, fill_coverage, NULL, sizeof(gs_coverage_rec));
}

/* stateCoverage(handle, minHits, minWeight, covered, whereMask, whereValue, op, bits) -> matched */
static napi_value js_state_coverage(napi_env env, napi_callback_info info) {
    CTX_ARGS(8, 8);
    uint32_t u[6]; /* minHits, covered, whereMask, whereValue, op, bits */
    static const int at[6] = {1, 3, 4, 5, 6, 7};
    for (int k = 0; k < 6; ++k) NAPI_CALL(env, napi_get_value_uint32(env, argv[at[k]], &u[k]));
    double min_weight = 0;
    NAPI_CALL(env, napi_get_value_double(env, argv[2], &min_weight));
    uint64_t matched = 0;
    int32_t rc = gs_state_coverage(ctx, u[0], (float)min_weight, u[1], u[2], u[3], u[4], u[5], &matched);
    return ret_u64(env, rc, matched);
}

/* ---- splat attributes: 1:1 wrappers of gs_attr_* and gs_state_attr ----------------------------------------------------------- */
/* (kind, p) of two arguments -> gs_attr; p: a Float32Array of four.  Returns 0 with a TypeError pending. */
static int get_attr(napi_env env, napi_value kind, napi_value p, gs_attr* a) {
    void* data = NULL;
    size_t len = 0;
    memset(a, 0, sizeof(*a));
    a->struct_size = sizeof(*a);
    if (napi_get_value_uint32(env, kind, &a->kind) != napi_ok || !get_bytes(env, p, &data, &len) || len < sizeof(a->p)) {
        napi_throw_type_error(env, NULL, "gsplat: an attribute is a kind (ATTR.*) and a Float32Array of four parameters");
        return 0;
    }
    memcpy(a->p, data, sizeof(a->p));
    return 1;
}

/* attrSummary(handle, kind, p, mask, value) -> {matched, nan, min, max} */
static napi_value js_attr_summary(napi_env env, napi_callback_info info) {
    CTX_ARGS(5, 5);
    gs_attr a;
    uint32_t mask = 0, value = 0;
    if (!get_attr(env, argv[1], argv[2], &a)) return NULL;
    NAPI_CALL(env, napi_get_value_uint32(env, argv[3], &mask));
    NAPI_CALL(env, napi_get_value_uint32(env, argv[4], &value));
    struct gs_attr_summary sm;
    int32_t rc = gs_attr_summary(ctx, &a, mask, value, &sm);
    if (rc != GS_OK) return throw_gs(env, rc);
    napi_value out;
    NAPI_CALL(env, napi_create_object(env, &out));
    set_num(env, out, "matched", (double)sm.matched);
    set_num(env, out, "nan", (double)sm.nan);
    set_num(env, out, "min", (double)sm.min);
    set_num(env, out, "max", (double)sm.max);
    return out;
}

/* attrHistogram(handle, kind, p, mask, value, lo, hi, bins) -> ArrayBuffer (bins + 3 u64: the bins, below, above, NaN) */
static napi_value js_attr_histogram(napi_env env, napi_callback_info info) {
    CTX_ARGS(8, 8);
    gs_attr a;
    uint32_t mask = 0, value = 0, bins = 0;
    double lo = 0, hi = 0;
    if (!get_attr(env, argv[1], argv[2], &a)) return NULL;
    NAPI_CALL(env, napi_get_value_uint32(env, argv[3], &mask));
    NAPI_CALL(env, napi_get_value_uint32(env, argv[4], &value));
    NAPI_CALL(env, napi_get_value_double(env, argv[5], &lo));
    NAPI_CALL(env, napi_get_value_double(env, argv[6], &hi));
    NAPI_CALL(env, napi_get_value_uint32(env, argv[7], &bins));
    void* dst = NULL;
    napi_value ab;
    NAPI_CALL(env, napi_create_arraybuffer(env, ((size_t)(bins <= 1024u ? bins : 0u) + 3) * sizeof(uint64_t), &dst, &ab)); /* (out of range: refused below) */
    int32_t rc = gs_attr_histogram(ctx, &a, mask, value, (float)lo, (float)hi, bins, (uint64_t*)dst);
    return rc == GS_OK ? ab : throw_gs(env, rc);
}

/* attrValues(handle, kind, p, mask, value) -> ArrayBuffer (one f32 per matching splat, ascending index order) */
static int32_t fill_attr_values(gs_ctx* ctx, const uint32_t* a, void* dst, uint64_t cap, uint64_t* n) { /* a: mask, value, then the gs_attr */
    return gs_attr_read(ctx, (const gs_attr*)(a + 2), a[0], a[1], (float*)dst, cap, n, NULL);
}
static napi_value js_attr_values(napi_env env, napi_callback_info info) {
    CTX_ARGS(5, 5);
    uint32_t w[2 + sizeof(gs_attr) / 4];
    gs_attr a;
    if (!get_attr(env, argv[1], argv[2], &a)) return NULL;
    NAPI_CALL(env, napi_get_value_uint32(env, argv[3], &w[0]));
    NAPI_CALL(env, napi_get_value_uint32(env, argv[4], &w[1]));
    memcpy(w + 2, &a, sizeof(a));
    return fill_arraybuffer(env, ctx, fill_attr_values, w, sizeof(float));
}

/* stateAttr(handle, kind, p, lo, hi, inside, whereMask, whereValue, op, bits) -> matched */
static napi_value js_state_attr(napi_env env, napi_callback_info info) {
    CTX_ARGS(10, 10);
    gs_attr a;
    if (!get_attr(env, argv[1], argv[2], &a)) return NULL;
    double lo = 0, hi = 0;
    NAPI_CALL(env, napi_get_value_double(env, argv[3], &lo));
    NAPI_CALL(env, napi_get_value_double(env, argv[4], &hi));
    uint32_t u[5]; /* inside, whereMask, whereValue, op, bits */
    for (int k = 0; k < 5; ++k) NAPI_CALL(env, napi_get_value_uint32(env, argv[5 + k], &u[k]));
    uint64_t matched = 0;
    int32_t rc = gs_state_attr(ctx, &a, (float)lo, (float)hi, u[0], u[1], u[2], u[3], u[4], &matched);
    return ret_u64(env, rc, matched);
}

/* ---- neighbourhoods: 1:1 wrappers of gs_neigh_* and gs_state_neigh -------------------------------------------------------- */
/* neighCount(handle, radius, limit, srcMask, srcValue, qryMask, qryValue, maxCandidates) -> {queried, sources, candidates, cells, cellEdge} */
static napi_value js_neigh_count(napi_env env, napi_callback_info info) {
    CTX_ARGS(8, 8);
    gs_neigh q;
    memset(&q, 0, sizeof(q));
    q.struct_size = sizeof(q);
    double radius = 0, budget = 0;
    NAPI_CALL(env, napi_get_value_double(env, argv[1], &radius));
    q.radius = (float)radius;
    uint32_t* u[5] = {&q.limit, &q.src_mask, &q.src_value, &q.qry_mask, &q.qry_value};
    for (int k = 0; k < 5; ++k) NAPI_CALL(env, napi_get_value_uint32(env, argv[2 + k], u[k]));
    NAPI_CALL(env, napi_get_value_double(env, argv[7], &budget));
    q.max_candidates = budget >= 1.0 ? (budget < 18446744073709549568.0 ? (uint64_t)budget : UINT64_MAX) : 0;
    gs_neigh_info ni;
    int32_t rc = gs_neigh_count(ctx, &q, &ni);
    if (rc != GS_OK) return throw_gs(env, rc);
    napi_value out, cells, v;
    NAPI_CALL(env, napi_create_object(env, &out));
    set_num(env, out, "queried", (double)ni.queried);
    set_num(env, out, "sources", (double)ni.sources);
    set_num(env, out, "candidates", (double)ni.candidates);
    set_num(env, out, "cellEdge", (double)ni.cell_edge);
    NAPI_CALL(env, napi_create_array_with_length(env, 3, &cells));
    for (uint32_t k = 0; k < 3; ++k) {
        NAPI_CALL(env, napi_create_uint32(env, ni.cells[k], &v));
        NAPI_CALL(env, napi_set_element(env, cells, k, v));
    }
    NAPI_CALL(env, napi_set_named_property(env, out, "cells", cells));
    return out;
}

/* neighRead(handle) -> ArrayBuffer (N counts, u32) */
static int32_t fill_neigh(gs_ctx* ctx, const uint32_t* a, void* dst, uint64_t cap, uint64_t* n) {
    (void)a;
    return gs_neigh_read(ctx, (uint32_t*)dst, cap, n);
}
static napi_value js_neigh_read(napi_env env, napi_callback_info info) {
    CTX_ARGS(1, 1);
    return fill_arraybuffer(env, ctx, fill_neigh, NULL, sizeof(uint32_t));
}

/* stateNeigh(handle, minCount, maxCount, inside, whereMask, whereValue, op, bits) -> matched */
static napi_value js_state_neigh(napi_env env, napi_callback_info info) {
    CTX_ARGS(8, 8);
    uint32_t u[7]; /* minCount, maxCount, inside, whereMask, whereValue, op, bits */
    for (int k = 0; k < 7; ++k) NAPI_CALL(env, napi_get_value_uint32(env, argv[1 + k], &u[k]));
    uint64_t matched = 0;
    int32_t rc = gs_state_neigh(ctx, u[0], u[1], u[2], u[3], u[4], u[5], u[6], &matched);
    return ret_u64(env, rc, matched);
}

/* ---- splat state (GS_FLAG_SPLAT_STATE): 1:1 wrappers of gs_state_* --------------------------------------------------------- */
static int get_f32x3_prop(napi_env env, napi_value obj, const char* name, float* out) {
    napi_value v, e;
    bool has = false;
    if (napi_has_named_property(env, obj, name, &has) != napi_ok || !has) return 0;
    if (napi_get_named_property(env, obj, name, &v) != napi_ok) return 0;
    for (uint32_t k = 0; k < 3; ++k) {
        double d;
        if (napi_get_element(env, v, k, &e) != napi_ok || napi_get_value_double(env, e, &d) != napi_ok) return 0;
        out[k] = (float)d;
    }
    return 1;
}

/* stateRegion(handle, {kind, a, b, x0, y0, x1, y1, uniforms, mask, whereMask, whereValue}, op, bits) -> matched */
static napi_value js_state_region(napi_env env, napi_callback_info info) {
    CTX_ARGS(4, 4);
    gs_region rg;
    memset(&rg, 0, sizeof(rg));
    rg.struct_size = sizeof(rg);
    if (!get_u32_prop(env, argv[1], "kind", &rg.kind)) {
        napi_throw_type_error(env, NULL, "gsplat.stateRegion: {kind} required");
        return NULL;
    }
    get_f32x3_prop(env, argv[1], "a", rg.a);
    get_f32x3_prop(env, argv[1], "b", rg.b);
    get_u32_prop(env, argv[1], "x0", &rg.x0);
    get_u32_prop(env, argv[1], "y0", &rg.y0);
    get_u32_prop(env, argv[1], "x1", &rg.x1);
    get_u32_prop(env, argv[1], "y1", &rg.y1);
    get_u32_prop(env, argv[1], "whereMask", &rg.where_mask);
    get_u32_prop(env, argv[1], "whereValue", &rg.where_value);
    napi_value v;
    bool has = false;
    void* data = NULL;
    size_t len = 0;
    if (napi_has_named_property(env, argv[1], "uniforms", &has) == napi_ok && has &&
        napi_get_named_property(env, argv[1], "uniforms", &v) == napi_ok && get_bytes(env, v, &data, &len)) {
        if (len < GS_UNIFORM_BYTES) { napi_throw_type_error(env, NULL, "gsplat.stateRegion: uniforms must be the 160-byte block"); return NULL; }
        rg.uniforms160 = data;
    }
    if (!get_mask_prop(env, argv[1], "stateRegion", &rg.mask)) return NULL;
    uint32_t op = 0, bits = 0;
    NAPI_CALL(env, napi_get_value_uint32(env, argv[2], &op));
    NAPI_CALL(env, napi_get_value_uint32(env, argv[3], &bits));
    uint64_t matched = 0;
    int32_t rc = gs_state_region(ctx, &rg, op, bits, &matched);
    return ret_u64(env, rc, matched);
}

/* stateIds(handle, ids (Uint32Array), op, bits) */
static napi_value js_state_ids(napi_env env, napi_callback_info info) {
    CTX_ARGS(4, 4);
    void* data = NULL;
    size_t len = 0;
    if (!get_bytes(env, argv[1], &data, &len) || len % 4 != 0) {
        napi_throw_type_error(env, NULL, "gsplat.stateIds: expects a Uint32Array of splat indices");
        return NULL;
    }
    uint32_t op = 0, bits = 0;
    NAPI_CALL(env, napi_get_value_uint32(env, argv[2], &op));
    NAPI_CALL(env, napi_get_value_uint32(env, argv[3], &bits));
    return ret_none(env, gs_state_ids(ctx, (const uint32_t*)data, (uint64_t)(len / 4), op, bits));
}

/* stateCount(handle, mask, value) -> count */
static napi_value js_state_count(napi_env env, napi_callback_info info) {
    CTX_ARGS(3, 3);
    uint32_t mask = 0, value = 0;
    NAPI_CALL(env, napi_get_value_uint32(env, argv[1], &mask));
    NAPI_CALL(env, napi_get_value_uint32(env, argv[2], &value));
    uint64_t count = 0;
    int32_t rc = gs_state_count(ctx, mask, value, &count);
    return ret_u64(env, rc, count);
}

/* readState(handle) -> ArrayBuffer (N bytes): the plane as it is now */
static napi_value js_read_state(napi_env env, napi_callback_info info) {
    CTX_ARGS(1, 1);
    const uint32_t which = GS_BUF_SPLAT_STATE;
    return fill_arraybuffer(env, ctx, fill_buffer, &which, 1);
}

/* writeState(handle, bytes (Uint8Array of N)) */
static napi_value js_write_state(napi_env env, napi_callback_info info) {
    CTX_ARGS(2, 2);
    void* data = NULL;
    size_t len = 0;
    if (!get_bytes(env, argv[1], &data, &len)) {
        napi_throw_type_error(env, NULL, "gsplat.writeState: expects a Uint8Array of N state bytes");
        return NULL;
    }
    return ret_none(env, gs_state_write(ctx, (const uint8_t*)data, (uint64_t)len));
}

/* ---- splat edits (gs_abi.h "splat edits") ---- */
static int get_filter(napi_env env, napi_value m, napi_value v, uint32_t* mask, uint32_t* value) {
    return napi_get_value_uint32(env, m, mask) == napi_ok && napi_get_value_uint32(env, v, value) == napi_ok;
}

/* listState(handle, mask, value) -> ArrayBuffer of u32 indices, ascending */
static napi_value js_list_state(napi_env env, napi_callback_info info) {
    CTX_ARGS(3, 3);
    uint32_t a[2] = {0, 0}; /* mask, value */
    if (!get_filter(env, argv[1], argv[2], &a[0], &a[1])) {
        napi_throw_type_error(env, NULL, "gsplat.listState: mask and value must be numbers");
        return NULL;
    }
    return fill_arraybuffer(env, ctx, fill_list, a, 4);
}

/* exportSplats(handle, mask, value) -> {n, records: ArrayBuffer (n x 320 B), ids: ArrayBuffer (n x u32)} */
static napi_value js_export_splats(napi_env env, napi_callback_info info) {
    CTX_ARGS(3, 3);
    uint32_t mask = 0, value = 0;
    if (!get_filter(env, argv[1], argv[2], &mask, &value)) {
        napi_throw_type_error(env, NULL, "gsplat.exportSplats: mask and value must be numbers");
        return NULL;
    }
    uint64_t n = 0;
    int32_t rc = gs_export_splats(ctx, mask, value, NULL, 0, &n, NULL);
    if (rc != GS_OK) return throw_gs(env, rc);
    void *rec = NULL, *ids = NULL;
    napi_value rab, iab, o;
    NAPI_CALL(env, napi_create_arraybuffer(env, (size_t)n * GS_SPLAT_RECORD_BYTES, &rec, &rab));
    NAPI_CALL(env, napi_create_arraybuffer(env, (size_t)n * 4, &ids, &iab));
    if (n) rc = gs_export_splats(ctx, mask, value, rec, n, &n, (uint32_t*)ids);
    if (rc != GS_OK) return throw_gs(env, rc);
    NAPI_CALL(env, napi_create_object(env, &o));
    set_num(env, o, "n", (double)n);
    napi_set_named_property(env, o, "records", rab);
    napi_set_named_property(env, o, "ids", iab);
    return o;
}

/* compact(handle, mask, value) -> ArrayBuffer of u32: ids[new index] = old index */
static napi_value js_compact(napi_env env, napi_callback_info info) {
    CTX_ARGS(3, 3);
    uint32_t mask = 0, value = 0;
    if (!get_filter(env, argv[1], argv[2], &mask, &value)) {
        napi_throw_type_error(env, NULL, "gsplat.compact: mask and value must be numbers");
        return NULL;
    }
    uint64_t kept = 0;
    gs_stats st;
    int32_t rc = gs_get_stats(ctx, &st);
    if (rc != GS_OK) return throw_gs(env, rc);
    uint32_t* ids = (uint32_t*)malloc(((size_t)st.num_gaussians + 1) * 4); /* gs_compact's capacity: N before the call */
    if (!ids) {
        napi_throw_error(env, NULL, "gsplat.compact: allocation failed");
        return NULL;
    }
    rc = gs_compact(ctx, mask, value, &kept, ids);
    if (rc != GS_OK) {
        free(ids);
        return throw_gs(env, rc);
    }
    void* dst = NULL;
    napi_value ab;
    if (napi_create_arraybuffer(env, (size_t)kept * 4, &dst, &ab) != napi_ok) {
        free(ids);
        napi_throw_error(env, NULL, "gsplat.compact: allocation failed");
        return NULL;
    }
    memcpy(dst, ids, (size_t)kept * 4);
    free(ids);
    return ab;
}

/* exportPly(handle, path, mask, value, shDegree) -> n written (gs_export_ply: streamed, no whole-scene host buffer) */
static napi_value js_export_ply(napi_env env, napi_callback_info info) {
    CTX_ARGS(5, 5);
    char path[4096];
    size_t len = 0;
    uint32_t mask = 0, value = 0;
    int32_t degree = 3;
    if (napi_get_value_string_utf8(env, argv[1], path, sizeof(path), &len) != napi_ok || !get_filter(env, argv[2], argv[3], &mask, &value) ||
        napi_get_value_int32(env, argv[4], &degree) != napi_ok) {
        napi_throw_type_error(env, NULL, "gsplat.exportPly: expects (handle, path, mask, value, shDegree)");
        return NULL;
    }
    uint64_t n = 0;
    int32_t rc = gs_export_ply(ctx, path, mask, value, degree, &n);
    return ret_u64(env, rc, n);
}

/* savePly(path, records (ArrayBuffer / typed array of n x 320 B), shDegree): gs_ply_save, no context */
static napi_value js_save_ply(napi_env env, napi_callback_info info) {
    ARGS(3);
    char path[4096];
    size_t len = 0, bytes = 0;
    void* data = NULL;
    int32_t degree = 3;
    if (argc < 3 || napi_get_value_string_utf8(env, argv[0], path, sizeof(path), &len) != napi_ok || !get_bytes(env, argv[1], &data, &bytes) ||
        bytes % GS_SPLAT_RECORD_BYTES != 0 || napi_get_value_int32(env, argv[2], &degree) != napi_ok) {
        napi_throw_type_error(env, NULL, "gsplat.savePly: expects (path, records of n x 320 bytes, shDegree)");
        return NULL;
    }
    return ret_none(env, gs_ply_save(path, data, (uint64_t)(bytes / GS_SPLAT_RECORD_BYTES), degree));
}

/* ---- splat transforms (gs_abi.h "splat transforms") ---- */
/* composeTransform(rot (4 numbers) | null, translate (3) | null, scale, pivot (3) | null) -> ArrayBuffer holding a gs_xform */
static int get_floats(napi_env env, napi_value v, float* out, uint32_t n) {
    bool is = false;
    if (napi_is_array(env, v, &is) != napi_ok) return 0;
    if (!is && (napi_is_typedarray(env, v, &is) != napi_ok || !is)) return 0;
    for (uint32_t k = 0; k < n; ++k) {
        napi_value e;
        double d;
        if (napi_get_element(env, v, k, &e) != napi_ok || napi_get_value_double(env, e, &d) != napi_ok) return 0;
        out[k] = (float)d;
    }
    return 1;
}
static int is_nullish(napi_env env, napi_value v) {
    napi_valuetype t;
    return napi_typeof(env, v, &t) == napi_ok && (t == napi_undefined || t == napi_null);
}
static napi_value js_compose_transform(napi_env env, napi_callback_info info) {
    ARGS(4);
    float rot[4] = {1.0f, 0.0f, 0.0f, 0.0f}, tr[3] = {0.0f, 0.0f, 0.0f}, pv[3];
    double scale = 1.0;
    int have_pivot = 0, ok = argc >= 4;
    if (ok && !is_nullish(env, argv[0])) ok = get_floats(env, argv[0], rot, 4);
    if (ok && !is_nullish(env, argv[1])) ok = get_floats(env, argv[1], tr, 3);
    if (ok && !is_nullish(env, argv[2])) ok = napi_get_value_double(env, argv[2], &scale) == napi_ok;
    if (ok && !is_nullish(env, argv[3])) ok = have_pivot = get_floats(env, argv[3], pv, 3);
    if (!ok) {
        napi_throw_type_error(env, NULL, "gsplat.composeTransform: expects (rotation[4] | null, translation[3] | null, scale | null, pivot[3] | null)");
        return NULL;
    }
    gs_xform x;
    int32_t rc = gs_xform_compose(rot, tr, (float)scale, have_pivot ? pv : NULL, &x);
    if (rc != GS_OK) return throw_gs(env, rc);
    void* dst = NULL;
    napi_value ab;
    NAPI_CALL(env, napi_create_arraybuffer(env, sizeof(x), &dst, &ab));
    memcpy(dst, &x, sizeof(x));
    return ab;
}

/* transformSplats(handle, xform (ArrayBuffer / typed array holding a gs_xform), mask, value) -> matched */
static napi_value js_transform_splats(napi_env env, napi_callback_info info) {
    CTX_ARGS(4, 4);
    void* data = NULL;
    size_t len = 0;
    uint32_t mask = 0, value = 0;
    if (!get_bytes(env, argv[1], &data, &len) || len != sizeof(gs_xform) || !get_filter(env, argv[2], argv[3], &mask, &value)) {
        napi_throw_type_error(env, NULL, "gsplat.transformSplats: expects (handle, the buffer composeTransform returned, mask, value)");
        return NULL;
    }
    gs_xform x;
    memcpy(&x, data, sizeof(x)); /* (a view may be unaligned) */
    uint64_t matched = 0;
    int32_t rc = gs_transform_splats(ctx, mask, value, &x, &matched);
    return ret_u64(env, rc, matched);
}

/* setOption(handle, key, value) */
static napi_value js_set_option(napi_env env, napi_callback_info info) {
    CTX_ARGS(3, 3);
    int32_t key = 0;
    double value = 0;
    NAPI_CALL(env, napi_get_value_int32(env, argv[1], &key));
    NAPI_CALL(env, napi_get_value_double(env, argv[2], &value));
    return ret_none(env, gs_set_option(ctx, key, (int64_t)value));
}

/* stats(handle) -> {numGaussians, numVisible, numIntersections, numProcessed, numTiles, sortPasses, frames, stageUs:[6], frameUs} */
static napi_value js_stats(napi_env env, napi_callback_info info) {
    CTX_ARGS(1, 1);
    gs_stats st;
    int32_t rc = gs_get_stats(ctx, &st);
    if (rc != GS_OK) return throw_gs(env, rc);
    napi_value o, arr;
    NAPI_CALL(env, napi_create_object(env, &o));
    set_num(env, o, "numGaussians", (double)st.num_gaussians);
    set_num(env, o, "numVisible", (double)st.num_visible);
    set_num(env, o, "numIntersections", (double)st.num_intersections);
    set_num(env, o, "numProcessed", (double)st.num_processed);
    set_num(env, o, "numTiles", (double)st.num_tiles);
    set_num(env, o, "sortPasses", (double)st.sort_passes);
    set_num(env, o, "frames", (double)st.frames);
    set_num(env, o, "frameUs", (double)st.frame_us);
    set_num(env, o, "numEvaluated", (double)st.num_evaluated);
    set_num(env, o, "depthOrdered", (double)st.depth_ordered);
    set_num(env, o, "tightBinning", (double)st.tight_binning);
    set_num(env, o, "graphFrames", (double)st.graph_frames);
    set_num(env, o, "capacity", (double)st.capacity);
    set_num(env, o, "maxIntersectionsSeen", (double)st.max_intersections_seen);
    set_num(env, o, "truncatedFrames", (double)st.truncated_frames);
    NAPI_CALL(env, napi_create_array_with_length(env, GS_STAGE_COUNT, &arr));
    for (uint32_t i = 0; i < GS_STAGE_COUNT; ++i) {
        napi_value n;
        napi_create_double(env, (double)st.stage_us[i], &n);
        napi_set_element(env, arr, i, n);
    }
    napi_set_named_property(env, o, "stageUs", arr);
    return o;
}

static napi_value js_slab(napi_env env, napi_callback_info info) {
    CTX_ARGS(1, 1);
    uint32_t b = 0, w = 0;
    int32_t rc = gs_slab_width(ctx, &b, &w);
    if (rc != GS_OK) return throw_gs(env, rc);
    napi_value o;
    NAPI_CALL(env, napi_create_object(env, &o));
    set_num(env, o, "begin", b);
    set_num(env, o, "width", w);
    return o;
}

/* loadPly(path) -> {n, degree, records: ArrayBuffer}: the native PackedGaussians (gs_ply_load) */
static napi_value js_load_ply(napi_env env, napi_callback_info info) {
    ARGS(1);
    char path[4096];
    size_t len = 0;
    if (argc < 1 || napi_get_value_string_utf8(env, argv[0], path, sizeof(path), &len) != napi_ok) {
        napi_throw_type_error(env, NULL, "gsplat.loadPly: path required");
        return NULL;
    }
    void* rec = NULL;
    uint64_t n = 0;
    int32_t degree = 0;
    int32_t rc = gs_ply_load(path, &rec, &n, &degree);
    if (rc != GS_OK) return throw_gs(env, rc);
    void* dst = NULL;
    napi_value ab, o;
    if (napi_create_arraybuffer(env, (size_t)n * GS_SPLAT_RECORD_BYTES, &dst, &ab) != napi_ok) {
        gs_ply_free(rec);
        napi_throw_error(env, NULL, "gsplat.loadPly: allocation failed");
        return NULL;
    }
    memcpy(dst, rec, (size_t)n * GS_SPLAT_RECORD_BYTES);
    gs_ply_free(rec);
    NAPI_CALL(env, napi_create_object(env, &o));
    set_num(env, o, "n", (double)n);
    set_num(env, o, "degree", (double)degree);
    napi_set_named_property(env, o, "records", ab);
    return o;
}

/* uploadPly(handle, path) -> n : the streaming loader (file -> pinned chunks -> device scene arrays, gs_upload_ply) */
static napi_value js_upload_ply(napi_env env, napi_callback_info info) {
    CTX_ARGS(2, 2);
    char path[4096];
    size_t len = 0;
    if (napi_get_value_string_utf8(env, argv[1], path, sizeof(path), &len) != napi_ok) {
        napi_throw_type_error(env, NULL, "gsplat.uploadPly: path required");
        return NULL;
    }
    uint64_t n = 0;
    int32_t rc = gs_upload_ply(ctx, path, &n);
    return ret_u64(env, rc, n);
}

/* hostAlloc(bytes) -> ArrayBuffer over page-locked memory (gs_host_alloc): a frame sink renderToSink copies into asynchronously */
static void finalize_pinned(napi_env env, void* data, void* hint) { (void)env; (void)hint; gs_host_free(data); }
static napi_value js_host_alloc(napi_env env, napi_callback_info info) {
    ARGS(1);
    double bytes = 0;
    if (argc < 1 || napi_get_value_double(env, argv[0], &bytes) != napi_ok || !(bytes > 0.0) || bytes > 17179869184.0) {
        napi_throw_type_error(env, NULL, "gsplat.hostAlloc: byte count required");
        return NULL;
    }
    void* p = NULL;
    int32_t rc = gs_host_alloc((uint64_t)bytes, &p);
    if (rc != GS_OK) return throw_gs(env, rc);
    napi_value ab;
    if (napi_create_external_arraybuffer(env, p, (size_t)bytes, finalize_pinned, NULL, &ab) != napi_ok) {
        gs_host_free(p);
        napi_throw_error(env, NULL, "gsplat.hostAlloc: napi_create_external_arraybuffer failed");
        return NULL;
    }
    return ab;
}

typedef struct {
    napi_async_work work;
    napi_deferred deferred;
    ctx_box* box;
    gs_ctx* ctx;
    uint64_t ticket;
    napi_ref sink_ref; /* keeps the sink alive until the copy has landed */
    int32_t rc;
    char err[512];
} sink_job;

static void sink_execute(napi_env env, void* data) {
    (void)env;
    sink_job* j = (sink_job*)data;
    j->rc = gs_wait_ticket(j->ctx, j->ticket);
    if (j->rc != GS_OK) { strncpy(j->err, gs_last_error(), sizeof(j->err) - 1); j->err[sizeof(j->err) - 1] = 0; }
}

static void sink_complete(napi_env env, napi_status status, void* data) {
    sink_job* j = (sink_job*)data;
    j->box->inflight--;
    finish_job(env, j->box, j->deferred, status, j->rc, j->err);
    napi_delete_reference(env, j->sink_ref);
    napi_delete_async_work(env, j->work);
    free(j);
}

/* renderToSink(handle, uniforms160, sink) -> Promise<void>: enqueues the frame and the copy of its pixels into `sink` NOW (on the
 * calling thread, without waiting: gs_render_host) and resolves when both are complete (gs_wait_ticket on a libuv worker).
 * Several may be outstanding: frame k+1 is enqueued while frame k is still being rendered and copied.  `sink`: ArrayBuffer or
 * view of at least height * slabWidth * 4 bytes, ideally from hostAlloc(). */
static napi_value js_render_to_sink(napi_env env, napi_callback_info info) {
    ARGS(3);
    ctx_box* box = argc >= 3 ? unbox(env, argv[0]) : NULL;
    if (!box) return NULL;
    if (!box->ctx || box->busy || box->destroy_pending) {
        napi_throw_error(env, NULL, "gsplat.renderToSink: the context is destroyed or owned by a renderAsync frame");
        return NULL;
    }
    void *udata = NULL, *sink = NULL;
    size_t ulen = 0, slen = 0;
    if (!get_bytes(env, argv[1], &udata, &ulen) || ulen < GS_UNIFORM_BYTES || !get_bytes(env, argv[2], &sink, &slen)) {
        napi_throw_type_error(env, NULL, "gsplat.renderToSink: need the 160-byte uniform block and a sink buffer");
        return NULL;
    }
    sink_job* j = (sink_job*)calloc(1, sizeof(sink_job));
    if (!j) { napi_throw_error(env, NULL, "gsplat.renderToSink: out of memory"); return NULL; }
    j->box = box;
    j->ctx = box->ctx;
    int32_t rc = gs_render_host(box->ctx, udata, sink, (uint64_t)slen, &j->ticket);
    if (rc != GS_OK) { free(j); return throw_gs(env, rc); }
    napi_value promise, name;
    if (napi_create_reference(env, argv[2], 1, &j->sink_ref) != napi_ok) {
        gs_wait_ticket(box->ctx, j->ticket); /* the copy must not outlive the buffer */
        free(j);
        napi_throw_error(env, NULL, "gsplat.renderToSink: N-API call failed");
        return NULL;
    }
    if (napi_create_promise(env, &j->deferred, &promise) != napi_ok ||
        napi_create_string_utf8(env, "gsplat.sink", NAPI_AUTO_LENGTH, &name) != napi_ok ||
        napi_create_async_work(env, NULL, name, sink_execute, sink_complete, j, &j->work) != napi_ok ||
        napi_queue_async_work(env, j->work) != napi_ok) {
        gs_wait_ticket(box->ctx, j->ticket);
        napi_delete_reference(env, j->sink_ref);
        free(j);
        napi_throw_error(env, NULL, "gsplat.renderToSink: N-API call failed");
        return NULL;
    }
    box->inflight++;
    return promise;
}

static napi_value init(napi_env env, napi_value exports) {
    static const struct { const char* name; napi_callback fn; } fns[] = {
        {"create", js_create},       {"destroy", js_destroy},         {"uploadSplats", js_upload},
        {"renderSync", js_render_sync}, {"renderAsync", js_render_async}, {"readRgba8", js_read_rgba8},
        {"readBuffer", js_read_buffer}, {"stats", js_stats},             {"slab", js_slab},
        {"loadPly", js_load_ply},    {"shareSplats", js_share},       {"uploadPly", js_upload_ply},
        {"hostAlloc", js_host_alloc}, {"renderToSink", js_render_to_sink}, {"pick", js_pick},
        {"stateRegion", js_state_region}, {"stateIds", js_state_ids},  {"stateCount", js_state_count},
        {"readState", js_read_state}, {"writeState", js_write_state},  {"setOption", js_set_option},
        {"listState", js_list_state}, {"exportSplats", js_export_splats}, {"compact", js_compact},
        {"exportPly", js_export_ply}, {"savePly", js_save_ply},
        {"composeTransform", js_compose_transform}, {"transformSplats", js_transform_splats},
        {"accumulateCoverage", js_coverage_accumulate}, {"resetCoverage", js_coverage_reset},
        {"readCoverage", js_coverage_read}, {"stateCoverage", js_state_coverage},
        {"attrSummary", js_attr_summary}, {"attrHistogram", js_attr_histogram},
        {"attrValues", js_attr_values}, {"stateAttr", js_state_attr},
        {"neighCount", js_neigh_count}, {"neighRead", js_neigh_read}, {"stateNeigh", js_state_neigh},
    };
    for (size_t i = 0; i < sizeof(fns) / sizeof(fns[0]); ++i) {
        napi_value f;
        if (napi_create_function(env, fns[i].name, NAPI_AUTO_LENGTH, fns[i].fn, NULL, &f) != napi_ok) return NULL;
        napi_set_named_property(env, exports, fns[i].name, f);
    }
    set_num(env, exports, "abiVersion", (double)gs_abi_version());
    set_num(env, exports, "FLAG_EXACT_BLEND", GS_FLAG_EXACT_BLEND);
    set_num(env, exports, "FLAG_F32_TAP", GS_FLAG_F32_TAP);
    set_num(env, exports, "FLAG_TIMING", GS_FLAG_TIMING);
    set_num(env, exports, "FLAG_AUX_OUTPUTS", GS_FLAG_AUX_OUTPUTS);
    set_num(env, exports, "FLAG_SPLAT_STATE", GS_FLAG_SPLAT_STATE);
    set_num(env, exports, "BUF_SPLAT_STATE", GS_BUF_SPLAT_STATE);
    set_num(env, exports, "OPT_SELECT_TINT", GS_OPT_SELECT_TINT);
    set_num(env, exports, "BUF_ALPHA_F32", GS_BUF_ALPHA_F32);
    set_num(env, exports, "BUF_DEPTH_F32", GS_BUF_DEPTH_F32);
    set_num(env, exports, "PICK_OK", GS_PICK_OK);
    set_num(env, exports, "PICK_OUTSIDE_SLAB", GS_PICK_OUTSIDE_SLAB);
    set_num(env, exports, "PICK_NONE", GS_PICK_NONE);
    set_num(env, exports, "PICK_MAX_QUERIES", GS_PICK_MAX_QUERIES);
    set_num(env, exports, "PICK_MAX_CONTRIB", GS_PICK_MAX_CONTRIB);
    set_num(env, exports, "COVERAGE_REC_BYTES", (double)sizeof(gs_coverage_rec));
    set_num(env, exports, "ATTR_COUNT", (double)GS_ATTR_COUNT);
    return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, init)
