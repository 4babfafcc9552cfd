/*
 * gs_napi.c -- plain-C N-API shim over include/gsplat/gs_abi.h (NAPI v4+, Node >= 12).
 *
 * This is the binding a Node host uses to put the MI355X rasterizer behind the reference's
 * TypeScript surface (Renderer / Camera / PackedGaussians, see ../../js).  It adds nothing to the
 * C ABI: every export is a 1:1 wrapper; HIP errors become thrown JS Errors / rejected Promises.
 * The per-frame call never blocks the JS thread: renderAsync() enqueues and waits in a libuv worker
 * (napi_async_work) and resolves a Promise, which is what Renderer.animate() awaits where the
 * reference awaits queue.onSubmittedWorkDone() (renderer.ts:404-587).
 *
 * A new 1:1 wrapper:
 *   1. CTX_ARGS(max, need) -- or ARGS(max) for a call without a context -- yields argc, argv and the unwrapped `ctx`.
 *   2. Read every argument through a reader (get_u32s, get_f64, get_path, get_uniforms, get_view, get_floats); each returns 0 with
 *      the exception pending, so the wrapper returns NULL.  A `complaint` {who, what} makes that a TypeError "gsplat.<who>: <what>";
 *      NULL leaves it at the generic "N-API call failed" Error.  Keep an index table only where the ABI's order is not the JS order.
 *   3. Call the gs_* function once.
 *   4. Return through ret_none / ret_u64, fill_arraybuffer (the ABI's size protocol) or copy_arraybuffer, and build an object of
 *      numbers from a num_row table with num_object (with_prop adds an ArrayBuffer or a num_array to it).
 *   5. Add the {"name", js_name} row to fns[] in init(), and the method to ../../js.
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

/* ---- errors ------------------------------------------------------------------------------------------------------------------ */
static napi_value throw_gs(napi_env env, int32_t rc) {
    char msg[640], code[16];
    const char* e = gs_last_error();
    snprintf(msg, sizeof(msg), "gsplat: %.608s", e && e[0] ? e : "error");
    snprintf(code, sizeof(code), "-%d", rc < 0 ? -rc : rc); /* the code property: "-1" .. "-8" */
    napi_throw_error(env, code, msg);
    return NULL;
}

/* Throws "gsplat.<who>: <what>" ("gsplat: <what>" without a who) as the class of `thrower`: napi_throw_type_error for an argument,
 * napi_throw_range_error, napi_throw_error.  Returns NULL, what a wrapper returns with an exception pending. */
typedef napi_status (*thrower)(napi_env, const char*, const char*);
static napi_value throw_who(napi_env env, thrower throw_as, const char* who, const char* what) {
    char msg[256];
    if (who) snprintf(msg, sizeof(msg), "gsplat.%s: %s", who, what);
    else snprintf(msg, sizeof(msg), "gsplat: %s", what);
    throw_as(env, NULL, msg);
    return NULL;
}

/* What a wrapper says about an argument it cannot read.  A reader given one throws it as a TypeError; given NULL it throws the
 * generic Error naming what it expected. */
typedef struct { const char *who, *what; } complaint;
static int refuse(napi_env env, const complaint* c, const char* expected) {
    char msg[96];
    snprintf(msg, sizeof(msg), "N-API call failed: %s expected", expected);
    if (c) throw_who(env, napi_throw_type_error, c->who, c->what);
    else napi_throw_error(env, NULL, msg);
    return 0;
}

/* ---- results ----------------------------------------------------------------------------------------------------------------- */
static void set_num(napi_env env, napi_value obj, const char* k, double v) {
    napi_value n;
    napi_create_double(env, v, &n);
    napi_set_named_property(env, obj, k, n);
}

/* what a wrapper of a call that reports nothing returns: throws on rc */
static napi_value ret_none(napi_env env, int32_t rc) { return rc == GS_OK ? NULL : throw_gs(env, rc); }
/* what a wrapper of a call that reports a count returns: throws on rc, otherwise the count as a double.  By address, so that
 * `return ret_u64(env, gs_call(ctx, ..., &n), &n)` reads n after the call whatever the order of evaluation. */
static napi_value ret_u64(napi_env env, int32_t rc, const uint64_t* value) {
    if (rc != GS_OK) return throw_gs(env, rc);
    napi_value out;
    NAPI_CALL(env, napi_create_double(env, (double)*value, &out));
    return out;
}

/* An object of numbers from a table of {name, value} rows: num_object(env, ROWS(rows)). */
typedef struct { const char* name; double value; } num_row;
#define ROWS(r) (r), sizeof(r) / sizeof((r)[0])
static napi_value num_object(napi_env env, const num_row* rows, size_t n) {
    napi_value o;
    NAPI_CALL(env, napi_create_object(env, &o));
    for (size_t i = 0; i < n; ++i) set_num(env, o, rows[i].name, rows[i].value);
    return o;
}
static napi_value num_array(napi_env env, const double* values, uint32_t n) {
    napi_value arr, v;
    NAPI_CALL(env, napi_create_array_with_length(env, n, &arr));
    for (uint32_t i = 0; i < n; ++i) {
        NAPI_CALL(env, napi_create_double(env, values[i], &v));
        NAPI_CALL(env, napi_set_element(env, arr, i, v));
    }
    return arr;
}
/* obj with obj[name] = v; NULL (the exception of whichever failed pending) when either is NULL */
static napi_value with_prop(napi_env env, napi_value obj, const char* name, napi_value v) {
    if (!obj || !v) return NULL;
    NAPI_CALL(env, napi_set_named_property(env, obj, name, v));
    return obj;
}
/* a new ArrayBuffer holding a copy of `bytes` bytes at src (the caller frees src either way); who: names the Error of a failed allocation */
static napi_value copy_arraybuffer(napi_env env, const void* src, size_t bytes, const char* who) {
    void* dst = NULL;
    napi_value ab;
    if (napi_create_arraybuffer(env, bytes, &dst, &ab) != napi_ok) return throw_who(env, napi_throw_error, who, "allocation failed");
    if (bytes) memcpy(dst, src, bytes);
    return ab;
}

/* ---- the context box -------------------------------------------------------------------------------------------------------- */
/* The external holds a box so that destroy() can null the context.  A gs_ctx is not re-entrant and the frame jobs work on it from
 * libuv workers: a renderAsync job owns it (`busy`), renderToSink jobs only wait for its tickets (`inflight`, several at a time).
 * While either is set every other call on the handle is refused, and destroy() and the finalizer are deferred to the last job's
 * completion.  Everything below runs on the JS thread, so the flags need no lock.  Only the box_* functions touch them; they keep
 *   busy and inflight never both set;  ctx != NULL while either is;  destroy_pending != 0 only while either is. */
typedef struct {
    gs_ctx* ctx;
    int busy;            /* a renderAsync job owns the context */
    int inflight;        /* renderToSink frames whose tickets are being waited for on workers (they only call gs_wait_ticket) */
    int destroy_pending; /* BOX_DESTROY or BOX_FINALIZE came meanwhile */
} ctx_box;
enum { BOX_DESTROY = 1, BOX_FINALIZE = 2 }; /* destroy(): the context goes, the box stays for the handle; the finalizer: both go */

/* The context for an ordinary call or for renderAsync: live and with no frame in flight, or NULL with an Error pending. */
static gs_ctx* box_idle_ctx(napi_env env, const ctx_box* b) {
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
/* The context for one more renderToSink frame: live, not owned by a renderAsync job and not about to be destroyed (other sink frames
 * may be in flight), or NULL with an Error pending. */
static gs_ctx* box_sink_ctx(napi_env env, const ctx_box* b) {
    if (!b->ctx || b->busy || b->destroy_pending)
        return (gs_ctx*)throw_who(env, napi_throw_error, "renderToSink", "the context is destroyed or owned by a renderAsync frame");
    return b->ctx;
}
/* A job takes the context it was given by box_idle_ctx (renderAsync) or box_sink_ctx (a sink frame) ... */
static void box_take_async(ctx_box* b) { b->busy = 1; }
static void box_take_sink(ctx_box* b) { b->inflight++; }
/* BOX_DESTROY or BOX_FINALIZE: now, or when the last job gives the context back (a finalizer outranks a destroy()). */
static void box_retire(ctx_box* b, int how) {
    if (b->busy || b->inflight) {
        if (how > b->destroy_pending) b->destroy_pending = how;
        return;
    }
    if (b->ctx) gs_destroy(b->ctx);
    b->ctx = NULL;
    if (how == BOX_FINALIZE) free(b);
}
/* ... and gives it back when it completes; the last one out carries out what was deferred.  The box may be gone afterwards. */
static void box_give_back(ctx_box* b, int sink) {
    if (sink) b->inflight--;
    else b->busy = 0;
    if (b->destroy_pending && !b->busy && !b->inflight) {
        const int how = b->destroy_pending;
        b->destroy_pending = 0;
        box_retire(b, how);
    }
}

static ctx_box* unbox_quiet(napi_env env, napi_value v) {
    void* p = NULL;
    return napi_get_value_external(env, v, &p) == napi_ok ? (ctx_box*)p : NULL;
}
static ctx_box* unbox(napi_env env, napi_value v) {
    ctx_box* b = unbox_quiet(env, v);
    if (!b) napi_throw_type_error(env, NULL, "gsplat: expected a context handle");
    return b;
}
static gs_ctx* unwrap(napi_env env, napi_value v) {
    ctx_box* b = unbox(env, v);
    return b ? box_idle_ctx(env, b) : NULL;
}
static void finalize_ctx(napi_env env, void* data, void* hint) {
    (void)env; (void)hint;
    box_retire((ctx_box*)data, BOX_FINALIZE);
}

/* Every wrapper's prologue.  ARGS(max): argc and argv[max], where N-API sets the arguments that were not given to undefined (so a
 * reader refuses them like any other wrong type).  CTX_ARGS(max, need) also yields the unwrapped context of argv[0] in
 * `ctx`, or returns: undefined for a call with fewer than `need` arguments, with unwrap's exception pending otherwise. */
#define ARGS(max)         \
    size_t argc = (max);  \
    napi_value argv[max]; \
    NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL))
#define CTX_ARGS(max, need)                                     \
    ARGS(max);                                                  \
    gs_ctx* ctx = argc >= (need) ? unwrap(env, argv[0]) : NULL; \
    if (!ctx) return NULL

/* ---- argument readers: each returns 0 with an exception pending (see `complaint`) ------------------------------------------- */
/* `count` consecutive u32 arguments from argv[first] (an i32 argument is read as u32 and cast: the same conversion modulo 2^32) */
static int get_u32s(napi_env env, const napi_value* argv, size_t first, size_t count, uint32_t* out, const complaint* c) {
    for (size_t k = 0; k < count; ++k)
        if (napi_get_value_uint32(env, argv[first + k], &out[k]) != napi_ok) return refuse(env, c, "a number");
    return 1;
}
static int get_f64(napi_env env, napi_value v, double* out, const complaint* c) {
    return napi_get_value_double(env, v, out) == napi_ok ? 1 : refuse(env, c, "a number");
}
/* a path of at most GS_PATH_MAX - 1 bytes; a longer one is cut there */
enum { GS_PATH_MAX = 4096 };
static int get_path(napi_env env, napi_value v, char* path, const complaint* c) {
    size_t len = 0;
    return napi_get_value_string_utf8(env, v, path, GS_PATH_MAX, &len) == napi_ok ? 1 : refuse(env, c, "a string");
}
/* bytes of an ArrayBuffer or of any TypedArray/Buffer view (quiet: 0 without an exception) */
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
/* a byte view of at least `min` bytes */
typedef struct { void* data; size_t len; } view;
static int get_view(napi_env env, napi_value v, size_t min, view* out, const complaint* c) {
    return get_bytes(env, v, &out->data, &out->len) && out->len >= min ? 1 : refuse(env, c, "a buffer of enough bytes");
}
/* the 160-byte uniform block */
static int get_uniforms(napi_env env, napi_value v, const void** u, const complaint* c) {
    view b;
    if (!get_view(env, v, GS_UNIFORM_BYTES, &b, c)) return 0;
    *u = b.data;
    return 1;
}
/* n floats from an array or a typed array (quiet: the callers have one message for several arguments, or none) */
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
static int get_flag(napi_env env, napi_value v) { /* a boolean; anything else is false */
    bool b = false;
    return napi_get_value_bool(env, v, &b) == napi_ok && b;
}
static int type_is(napi_env env, napi_value v, napi_valuetype want) {
    napi_valuetype t;
    return napi_typeof(env, v, &t) == napi_ok && t == want;
}
static int is_nullish(napi_env env, napi_value v) { return type_is(env, v, napi_undefined) || type_is(env, v, napi_null); }

/* Optional properties of an options object: 1 and the value when obj has a usable `name`, 0 (quiet, *out as it was) otherwise. */
static int get_prop(napi_env env, napi_value obj, const char* name, napi_value* v) {
    bool has = false;
    return napi_has_named_property(env, obj, name, &has) == napi_ok && has && napi_get_named_property(env, obj, name, v) == napi_ok;
}
static int get_u32_prop(napi_env env, napi_value obj, const char* name, uint32_t* out) {
    napi_value v;
    double d;
    if (!get_prop(env, obj, name, &v) || napi_get_value_double(env, v, &d) != napi_ok) return 0;
    *out = (uint32_t)d;
    return 1;
}
static int get_f32x3_prop(napi_env env, napi_value obj, const char* name, float* out) {
    napi_value v;
    float f[3];
    if (!get_prop(env, obj, name, &v) || !get_floats(env, v, f, 3)) return 0;
    memcpy(out, f, sizeof(f));
    return 1;
}
/* obj.mask (bytes) with obj.maskWidth and obj.maskHeight: the mask covers the CANVAS (the JS Renderer passes its canvas size),
 * checked against the bytes given.  *mask stays as it is without a usable obj.mask.  Returns 0 with a TypeError pending. */
static int get_mask_prop(napi_env env, napi_value obj, const char* who, const uint8_t** mask) {
    napi_value v;
    void* data = NULL;
    size_t len = 0;
    if (!get_prop(env, obj, "mask", &v) || !get_bytes(env, v, &data, &len)) return 1;
    uint32_t cw = 0, ch = 0;
    if (!get_u32_prop(env, obj, "maskWidth", &cw) || !get_u32_prop(env, obj, "maskHeight", &ch) || (double)len < (double)cw * (double)ch) {
        throw_who(env, napi_throw_type_error, who, "mask needs maskWidth, maskHeight and width * height bytes");
        return 0;
    }
    *mask = (const uint8_t*)data;
    return 1;
}

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

/* ---- contexts and frames ----------------------------------------------------------------------------------------------------- */
/* create({width,height,tileSize,device,colBegin,colEnd,flags,maxIntersections}) -> handle */
static napi_value js_create(napi_env env, napi_callback_info info) {
    ARGS(1);
    gs_config cfg = {.struct_size = sizeof(cfg), .tile_size = 16};
    uint32_t dev = 0, maxi = 0;
    if (argc < 1 || !get_u32_prop(env, argv[0], "width", &cfg.width) || !get_u32_prop(env, argv[0], "height", &cfg.height))
        return throw_who(env, napi_throw_type_error, "create", "{width, height} required");
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
    if (!box) { gs_destroy(ctx); return throw_who(env, napi_throw_error, "create", "out of memory"); }
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

/* destroy(handle): anything that is not a handle is ignored */
static napi_value js_destroy(napi_env env, napi_callback_info info) {
    ARGS(1);
    ctx_box* box = argc >= 1 ? unbox_quiet(env, argv[0]) : NULL;
    if (box) box_retire(box, BOX_DESTROY);
    return NULL;
}

/* uploadSplats(handle, bytes, n) */
static napi_value js_upload(napi_env env, napi_callback_info info) {
    CTX_ARGS(3, 3);
    static const complaint bad = {"uploadSplats", "need n*320 bytes"};
    view rec;
    double n = 0;
    if (!get_view(env, argv[1], 0, &rec, &bad) || !get_f64(env, argv[2], &n, &bad)) return NULL;
    if (!(n >= 0.0) || n != (double)(uint64_t)n || n >= 2147483648.0 || (double)rec.len < n * GS_SPLAT_RECORD_BYTES)
        return throw_who(env, napi_throw_type_error, bad.who, bad.what);
    return ret_none(env, gs_upload_splats(ctx, rec.data, (uint64_t)n));
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
    static const complaint bad = {"render", "need the 160-byte uniform block"};
    const void* u = NULL;
    if (!get_uniforms(env, argv[1], &u, &bad)) return NULL;
    int32_t rc = argc >= 3 && get_flag(env, argv[2]) ? gs_render_debug(ctx, u) : gs_render(ctx, u);
    if (rc == GS_OK) rc = gs_wait(ctx);
    return ret_none(env, rc);
}

/* One frame on a libuv worker, for renderAsync (render `uniforms`, wait) and for renderToSink (wait for `ticket`). */
typedef struct {
    napi_async_work work;
    napi_deferred deferred;
    ctx_box* box;
    gs_ctx* ctx;
    napi_ref sink_ref; /* a renderToSink frame: keeps the sink alive until the copy has landed; NULL: a renderAsync frame */
    uint64_t ticket;
    unsigned char uniforms[GS_UNIFORM_BYTES];
    int32_t rc;
    char err[512];
} frame_job;

static void job_execute(napi_env env, void* data) {
    (void)env;
    frame_job* j = (frame_job*)data;
    if (j->sink_ref) j->rc = gs_wait_ticket(j->ctx, j->ticket);
    else {
        j->rc = gs_render(j->ctx, j->uniforms);
        if (j->rc == GS_OK) j->rc = gs_wait(j->ctx);
    }
    if (j->rc != GS_OK) { /* gs_last_error is thread-local: capture it on the worker thread */
        strncpy(j->err, gs_last_error(), sizeof(j->err) - 1);
        j->err[sizeof(j->err) - 1] = 0;
    }
}

/* settles a job's promise */
static void finish_job(napi_env env, napi_deferred deferred, napi_status status, int32_t rc, const char* err) {
    napi_value v;
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
    box_give_back(j->box, j->sink_ref != NULL); /* first: a deferred destroy() happens before the promise settles */
    finish_job(env, j->deferred, status, j->rc, j->err);
    if (j->sink_ref) napi_delete_reference(env, j->sink_ref);
    napi_delete_async_work(env, j->work);
    free(j);
}

/* Starts a job whose box, ctx and uniforms or ticket are filled in; sink: the buffer of a renderToSink frame, NULL for renderAsync.
 * Returns the promise.  On a failure it undoes what it did -- after waiting for a sink frame's ticket, because the copy that
 * gs_render_host enqueued must not outlive the buffer --, frees j and returns NULL with an Error pending. */
static napi_value start_job(napi_env env, frame_job* j, napi_value sink, const char* who) {
    napi_value promise, name;
    const char* what = "N-API call failed";
    if ((!sink || napi_create_reference(env, sink, 1, &j->sink_ref) == napi_ok) && napi_create_promise(env, &j->deferred, &promise) == napi_ok &&
        napi_create_string_utf8(env, sink ? "gsplat.sink" : "gsplat.frame", NAPI_AUTO_LENGTH, &name) == napi_ok &&
        napi_create_async_work(env, NULL, name, job_execute, job_complete, j, &j->work) == napi_ok) {
        if (sink) box_take_sink(j->box);
        else box_take_async(j->box);
        if (napi_queue_async_work(env, j->work) == napi_ok) return promise;
        box_give_back(j->box, sink != NULL);
        if (!sink) what = "napi_queue_async_work failed";
    }
    if (sink) gs_wait_ticket(j->ctx, j->ticket);
    if (j->sink_ref) napi_delete_reference(env, j->sink_ref);
    if (j->work) napi_delete_async_work(env, j->work);
    free(j);
    return throw_who(env, napi_throw_error, who, what);
}

/* renderAsync(handle, uniforms160) -> Promise<void> */
static napi_value js_render_async(napi_env env, napi_callback_info info) {
    CTX_ARGS(2, 2);
    static const complaint bad = {"renderAsync", "need the 160-byte uniform block"};
    const void* u = NULL;
    if (!get_uniforms(env, argv[1], &u, &bad)) return NULL;
    frame_job* j = (frame_job*)calloc(1, sizeof(frame_job));
    if (!j) return throw_who(env, napi_throw_error, "renderAsync", "out of memory");
    j->box = unbox(env, argv[0]);
    j->ctx = ctx;
    memcpy(j->uniforms, u, GS_UNIFORM_BYTES);
    return start_job(env, j, NULL, "renderAsync");
}

/* renderToSink(handle, uniforms160, sink) -> Promise<void>: enqueues the frame and the copy of its pixels into `sink` NOW (on the
 * calling thread, without waiting: gs_render_host) and resolves when both are complete (gs_wait_ticket on a libuv worker).
 * Several may be outstanding: frame k+1 is enqueued while frame k is still being rendered and copied.  `sink`: ArrayBuffer or
 * view of at least height * slabWidth * 4 bytes, ideally from hostAlloc(). */
static napi_value js_render_to_sink(napi_env env, napi_callback_info info) {
    ARGS(3);
    static const complaint bad = {"renderToSink", "need the 160-byte uniform block and a sink buffer"};
    ctx_box* box = argc >= 3 ? unbox(env, argv[0]) : NULL;
    gs_ctx* ctx = box ? box_sink_ctx(env, box) : NULL;
    if (!ctx) return NULL;
    const void* u = NULL;
    view sink;
    if (!get_uniforms(env, argv[1], &u, &bad) || !get_view(env, argv[2], 0, &sink, &bad)) return NULL;
    frame_job* j = (frame_job*)calloc(1, sizeof(frame_job));
    if (!j) return throw_who(env, napi_throw_error, "renderToSink", "out of memory");
    j->box = box;
    j->ctx = ctx;
    int32_t rc = gs_render_host(ctx, u, sink.data, (uint64_t)sink.len, &j->ticket);
    if (rc != GS_OK) { free(j); return throw_gs(env, rc); }
    return start_job(env, j, argv[2], "renderToSink");
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
    uint32_t which = 0;
    if (!get_u32s(env, argv, 1, 1, &which, NULL)) return NULL;
    return fill_arraybuffer(env, ctx, fill_buffer, &which, 1);
}

/* pick(handle, queries ( Uint32Array x,y pairs ), maxContrib) -> {results: ArrayBuffer (48 bytes per query), contrib: ArrayBuffer | null} */
static napi_value js_pick(napi_env env, napi_callback_info info) {
    CTX_ARGS(3, 2);
    static const complaint bad = {NULL, "pick expects a Uint32Array of x,y pairs"};
    view q;
    if (!get_view(env, argv[1], 0, &q, &bad)) return NULL;
    if (q.len % sizeof(gs_pick_query) != 0) return throw_who(env, napi_throw_type_error, bad.who, bad.what);
    uint32_t max_contrib = 0;
    if (argc >= 3 && !get_u32s(env, argv, 2, 1, &max_contrib, NULL)) return NULL;
    const size_t n = q.len / sizeof(gs_pick_query);
    if (n == 0 || n > GS_PICK_MAX_QUERIES || max_contrib > GS_PICK_MAX_CONTRIB) /* (they size the buffers below) */
        return throw_who(env, napi_throw_range_error, NULL, "pick takes 1..65536 queries and maxContrib 0..256");
    void *res = NULL, *con = NULL;
    napi_value res_ab, con_ab;
    NAPI_CALL(env, napi_create_arraybuffer(env, n * sizeof(gs_pick_result), &res, &res_ab));
    if (max_contrib) NAPI_CALL(env, napi_create_arraybuffer(env, n * max_contrib * sizeof(gs_pick_contrib), &con, &con_ab));
    else NAPI_CALL(env, napi_get_null(env, &con_ab));
    int32_t rc = gs_pick(ctx, (const gs_pick_query*)q.data, (uint32_t)n, (gs_pick_result*)res, max_contrib, (gs_pick_contrib*)con);
    if (rc != GS_OK) return throw_gs(env, rc);
    return with_prop(env, with_prop(env, num_object(env, NULL, 0), "results", res_ab), "contrib", con_ab);
}

/* ---- coverage: 1:1 wrappers of gs_coverage_* and gs_state_coverage ---------------------------------------------------------- */
/* accumulateCoverage(handle, region | null) -> pixels; region = {x0, y0, x1, y1, mask, maskWidth, maskHeight} (canvas pixels) */
static napi_value js_coverage_accumulate(napi_env env, napi_callback_info info) {
    CTX_ARGS(2, 1);
    gs_cover_region rg = {.struct_size = sizeof(rg)};
    const int have = argc >= 2 && type_is(env, argv[1], napi_object);
    if (have) {
        if (!get_u32_prop(env, argv[1], "x0", &rg.x0) || !get_u32_prop(env, argv[1], "y0", &rg.y0) || !get_u32_prop(env, argv[1], "x1", &rg.x1) ||
            !get_u32_prop(env, argv[1], "y1", &rg.y1))
            return throw_who(env, napi_throw_type_error, "accumulateCoverage", "{x0, y0, x1, y1} required");
        if (!get_mask_prop(env, argv[1], "accumulateCoverage", &rg.mask)) return NULL;
    }
    uint64_t pixels = 0;
    return ret_u64(env, gs_coverage_accumulate(ctx, have ? &rg : NULL, &pixels), &pixels);
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
    uint32_t min_hits = 0, u[5]; /* covered, whereMask, whereValue, op, bits */
    double min_weight = 0;
    if (!get_u32s(env, argv, 1, 1, &min_hits, NULL) || !get_u32s(env, argv, 3, 5, u, NULL) || !get_f64(env, argv[2], &min_weight, NULL)) return NULL;
    uint64_t matched = 0;
    return ret_u64(env, gs_state_coverage(ctx, min_hits, (float)min_weight, u[0], u[1], u[2], u[3], u[4], &matched), &matched);
}

/* ---- splat attributes: 1:1 wrappers of gs_attr_* and gs_state_attr ----------------------------------------------------------- */
/* (kind, p) at argv[first] and argv[first + 1] -> gs_attr; p: a Float32Array of four */
static int get_attr(napi_env env, const napi_value* argv, size_t first, gs_attr* a) {
    static const complaint bad = {NULL, "an attribute is a kind (ATTR.*) and a Float32Array of four parameters"};
    view p;
    *a = (gs_attr){.struct_size = sizeof(*a)};
    if (!get_u32s(env, argv, first, 1, &a->kind, &bad) || !get_view(env, argv[first + 1], sizeof(a->p), &p, &bad)) return 0;
    memcpy(a->p, p.data, sizeof(a->p));
    return 1;
}

/* attrSummary(handle, kind, p, mask, value) -> {matched, nan, min, max} */
static napi_value js_attr_summary(napi_env env, napi_callback_info info) {
    CTX_ARGS(5, 5);
    gs_attr a;
    uint32_t f[2]; /* mask, value */
    if (!get_attr(env, argv, 1, &a) || !get_u32s(env, argv, 3, 2, f, NULL)) return NULL;
    struct gs_attr_summary sm;
    int32_t rc = gs_attr_summary(ctx, &a, f[0], f[1], &sm);
    if (rc != GS_OK) return throw_gs(env, rc);
    const num_row rows[] = {{"matched", (double)sm.matched}, {"nan", (double)sm.nan}, {"min", (double)sm.min}, {"max", (double)sm.max}};
    return num_object(env, ROWS(rows));
}

/* attrHistogram(handle, kind, p, mask, value, lo, hi, bins) -> ArrayBuffer (bins + 3 u64: the bins, below, above, NaN) */
static napi_value js_attr_histogram(napi_env env, napi_callback_info info) {
    CTX_ARGS(8, 8);
    gs_attr a;
    uint32_t f[2], bins = 0; /* f: mask, value */
    double lo = 0, hi = 0;
    if (!get_attr(env, argv, 1, &a) || !get_u32s(env, argv, 3, 2, f, NULL) || !get_f64(env, argv[5], &lo, NULL) || !get_f64(env, argv[6], &hi, NULL) ||
        !get_u32s(env, argv, 7, 1, &bins, NULL))
        return NULL;
    void* dst = NULL;
    napi_value ab;
    NAPI_CALL(env, napi_create_arraybuffer(env, ((size_t)(bins <= 1024u ? bins : 0u) + 3) * sizeof(uint64_t), &dst, &ab)); /* (out of range: refused below) */
    int32_t rc = gs_attr_histogram(ctx, &a, f[0], f[1], (float)lo, (float)hi, bins, (uint64_t*)dst);
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
    if (!get_attr(env, argv, 1, &a) || !get_u32s(env, argv, 3, 2, w, NULL)) return NULL;
    memcpy(w + 2, &a, sizeof(a));
    return fill_arraybuffer(env, ctx, fill_attr_values, w, sizeof(float));
}

/* stateAttr(handle, kind, p, lo, hi, inside, whereMask, whereValue, op, bits) -> matched */
static napi_value js_state_attr(napi_env env, napi_callback_info info) {
    CTX_ARGS(10, 10);
    gs_attr a;
    double lo = 0, hi = 0;
    uint32_t u[5]; /* inside, whereMask, whereValue, op, bits */
    if (!get_attr(env, argv, 1, &a) || !get_f64(env, argv[3], &lo, NULL) || !get_f64(env, argv[4], &hi, NULL) || !get_u32s(env, argv, 5, 5, u, NULL))
        return NULL;
    uint64_t matched = 0;
    return ret_u64(env, gs_state_attr(ctx, &a, (float)lo, (float)hi, u[0], u[1], u[2], u[3], u[4], &matched), &matched);
}

/* ---- neighbourhoods: 1:1 wrappers of gs_neigh_* and gs_state_neigh -------------------------------------------------------- */
/* neighCount(handle, radius, limit, srcMask, srcValue, qryMask, qryValue, maxCandidates) -> {queried, sources, candidates, cells, cellEdge} */
static napi_value js_neigh_count(napi_env env, napi_callback_info info) {
    CTX_ARGS(8, 8);
    gs_neigh q = {.struct_size = sizeof(q)};
    double radius = 0, budget = 0;
    uint32_t u[5]; /* limit, srcMask, srcValue, qryMask, qryValue */
    if (!get_f64(env, argv[1], &radius, NULL) || !get_u32s(env, argv, 2, 5, u, NULL) || !get_f64(env, argv[7], &budget, NULL)) return NULL;
    q.radius = (float)radius;
    q.limit = u[0], q.src_mask = u[1], q.src_value = u[2], q.qry_mask = u[3], q.qry_value = u[4];
    q.max_candidates = budget >= 1.0 ? (budget < 18446744073709549568.0 ? (uint64_t)budget : UINT64_MAX) : 0;
    gs_neigh_info ni;
    int32_t rc = gs_neigh_count(ctx, &q, &ni);
    if (rc != GS_OK) return throw_gs(env, rc);
    const num_row rows[] = {{"queried", (double)ni.queried}, {"sources", (double)ni.sources}, {"candidates", (double)ni.candidates},
                            {"cellEdge", (double)ni.cell_edge}};
    const double cells[3] = {ni.cells[0], ni.cells[1], ni.cells[2]};
    return with_prop(env, num_object(env, ROWS(rows)), "cells", num_array(env, cells, 3));
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
    if (!get_u32s(env, argv, 1, 7, u, NULL)) return NULL;
    uint64_t matched = 0;
    return ret_u64(env, gs_state_neigh(ctx, u[0], u[1], u[2], u[3], u[4], u[5], u[6], &matched), &matched);
}

/* ---- splat state (GS_FLAG_SPLAT_STATE): 1:1 wrappers of gs_state_* --------------------------------------------------------- */
/* stateRegion(handle, {kind, a, b, x0, y0, x1, y1, uniforms, mask, whereMask, whereValue}, op, bits) -> matched */
static napi_value js_state_region(napi_env env, napi_callback_info info) {
    CTX_ARGS(4, 4);
    static const complaint bad_uniforms = {"stateRegion", "uniforms must be the 160-byte block"};
    gs_region rg = {.struct_size = sizeof(rg)};
    if (!get_u32_prop(env, argv[1], "kind", &rg.kind)) return throw_who(env, napi_throw_type_error, "stateRegion", "{kind} required");
    get_f32x3_prop(env, argv[1], "a", rg.a);
    get_f32x3_prop(env, argv[1], "b", rg.b);
    get_u32_prop(env, argv[1], "x0", &rg.x0);
    get_u32_prop(env, argv[1], "y0", &rg.y0);
    get_u32_prop(env, argv[1], "x1", &rg.x1);
    get_u32_prop(env, argv[1], "y1", &rg.y1);
    get_u32_prop(env, argv[1], "whereMask", &rg.where_mask);
    get_u32_prop(env, argv[1], "whereValue", &rg.where_value);
    napi_value v;
    void* data = NULL;
    size_t len = 0;
    if (get_prop(env, argv[1], "uniforms", &v) && get_bytes(env, v, &data, &len) && !get_uniforms(env, v, &rg.uniforms160, &bad_uniforms)) return NULL;
    if (!get_mask_prop(env, argv[1], "stateRegion", &rg.mask)) return NULL;
    uint32_t o[2]; /* op, bits */
    if (!get_u32s(env, argv, 2, 2, o, NULL)) return NULL;
    uint64_t matched = 0;
    return ret_u64(env, gs_state_region(ctx, &rg, o[0], o[1], &matched), &matched);
}

/* stateIds(handle, ids (Uint32Array), op, bits) */
static napi_value js_state_ids(napi_env env, napi_callback_info info) {
    CTX_ARGS(4, 4);
    static const complaint bad = {"stateIds", "expects a Uint32Array of splat indices"};
    view ids;
    if (!get_view(env, argv[1], 0, &ids, &bad)) return NULL;
    if (ids.len % 4 != 0) return throw_who(env, napi_throw_type_error, bad.who, bad.what);
    uint32_t o[2]; /* op, bits */
    if (!get_u32s(env, argv, 2, 2, o, NULL)) return NULL;
    return ret_none(env, gs_state_ids(ctx, (const uint32_t*)ids.data, (uint64_t)(ids.len / 4), o[0], o[1]));
}

/* stateCount(handle, mask, value) -> count */
static napi_value js_state_count(napi_env env, napi_callback_info info) {
    CTX_ARGS(3, 3);
    uint32_t f[2]; /* mask, value */
    if (!get_u32s(env, argv, 1, 2, f, NULL)) return NULL;
    uint64_t count = 0;
    return ret_u64(env, gs_state_count(ctx, f[0], f[1], &count), &count);
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
    static const complaint bad = {"writeState", "expects a Uint8Array of N state bytes"};
    view plane;
    if (!get_view(env, argv[1], 0, &plane, &bad)) return NULL;
    return ret_none(env, gs_state_write(ctx, (const uint8_t*)plane.data, (uint64_t)plane.len));
}

/* ---- splat edits (gs_abi.h "splat edits") ---- */
/* listState(handle, mask, value) -> ArrayBuffer of u32 indices, ascending */
static napi_value js_list_state(napi_env env, napi_callback_info info) {
    CTX_ARGS(3, 3);
    static const complaint bad = {"listState", "mask and value must be numbers"};
    uint32_t f[2]; /* mask, value */
    if (!get_u32s(env, argv, 1, 2, f, &bad)) return NULL;
    return fill_arraybuffer(env, ctx, fill_list, f, 4);
}

/* exportSplats(handle, mask, value) -> {n, records: ArrayBuffer (n x 320 B), ids: ArrayBuffer (n x u32)} */
static napi_value js_export_splats(napi_env env, napi_callback_info info) {
    CTX_ARGS(3, 3);
    static const complaint bad = {"exportSplats", "mask and value must be numbers"};
    uint32_t f[2]; /* mask, value */
    if (!get_u32s(env, argv, 1, 2, f, &bad)) return NULL;
    uint64_t n = 0;
    int32_t rc = gs_export_splats(ctx, f[0], f[1], NULL, 0, &n, NULL);
    if (rc != GS_OK) return throw_gs(env, rc);
    void *rec = NULL, *ids = NULL;
    napi_value rab, iab;
    NAPI_CALL(env, napi_create_arraybuffer(env, (size_t)n * GS_SPLAT_RECORD_BYTES, &rec, &rab));
    NAPI_CALL(env, napi_create_arraybuffer(env, (size_t)n * 4, &ids, &iab));
    if (n) rc = gs_export_splats(ctx, f[0], f[1], rec, n, &n, (uint32_t*)ids);
    if (rc != GS_OK) return throw_gs(env, rc);
    const num_row rows[] = {{"n", (double)n}};
    return with_prop(env, with_prop(env, num_object(env, ROWS(rows)), "records", rab), "ids", iab);
}

/* compact(handle, mask, value) -> ArrayBuffer of u32: ids[new index] = old index */
static napi_value js_compact(napi_env env, napi_callback_info info) {
    CTX_ARGS(3, 3);
    static const complaint bad = {"compact", "mask and value must be numbers"};
    uint32_t f[2]; /* mask, value */
    if (!get_u32s(env, argv, 1, 2, f, &bad)) return NULL;
    uint64_t kept = 0;
    gs_stats st;
    int32_t rc = gs_get_stats(ctx, &st);
    if (rc != GS_OK) return throw_gs(env, rc);
    uint32_t* ids = (uint32_t*)malloc(((size_t)st.num_gaussians + 1) * 4); /* gs_compact's capacity: N before the call */
    if (!ids) return throw_who(env, napi_throw_error, "compact", "allocation failed");
    rc = gs_compact(ctx, f[0], f[1], &kept, ids);
    napi_value ab = rc == GS_OK ? copy_arraybuffer(env, ids, (size_t)kept * 4, "compact") : throw_gs(env, rc);
    free(ids);
    return ab;
}

/* exportPly(handle, path, mask, value, shDegree) -> n written (gs_export_ply: streamed, no whole-scene host buffer) */
static napi_value js_export_ply(napi_env env, napi_callback_info info) {
    CTX_ARGS(5, 5);
    static const complaint bad = {"exportPly", "expects (handle, path, mask, value, shDegree)"};
    char path[GS_PATH_MAX];
    uint32_t u[3]; /* mask, value, shDegree */
    if (!get_path(env, argv[1], path, &bad) || !get_u32s(env, argv, 2, 3, u, &bad)) return NULL;
    uint64_t n = 0;
    return ret_u64(env, gs_export_ply(ctx, path, u[0], u[1], (int32_t)u[2], &n), &n);
}

/* savePly(path, records (ArrayBuffer / typed array of n x 320 B), shDegree): gs_ply_save, no context */
static napi_value js_save_ply(napi_env env, napi_callback_info info) {
    ARGS(3);
    static const complaint bad = {"savePly", "expects (path, records of n x 320 bytes, shDegree)"};
    char path[GS_PATH_MAX];
    view rec;
    uint32_t degree = 3;
    if (!get_path(env, argv[0], path, &bad) || !get_view(env, argv[1], 0, &rec, &bad)) return NULL;
    if (rec.len % GS_SPLAT_RECORD_BYTES != 0) return throw_who(env, napi_throw_type_error, bad.who, bad.what);
    if (!get_u32s(env, argv, 2, 1, &degree, &bad)) return NULL;
    return ret_none(env, gs_ply_save(path, rec.data, (uint64_t)(rec.len / GS_SPLAT_RECORD_BYTES), (int32_t)degree));
}

/* ---- splat transforms (gs_abi.h "splat transforms") ---- */
/* composeTransform(rot (4 numbers) | null, translate (3) | null, scale, pivot (3) | null) -> ArrayBuffer holding a gs_xform */
static napi_value js_compose_transform(napi_env env, napi_callback_info info) {
    ARGS(4);
    static const complaint bad = {"composeTransform", "expects (rotation[4] | null, translation[3] | null, scale | null, pivot[3] | null)"};
    float rot[4] = {1.0f, 0.0f, 0.0f, 0.0f}, tr[3] = {0.0f, 0.0f, 0.0f}, pv[3];
    double scale = 1.0;
    int have_pivot = 0, ok = argc >= 4;
    if (ok && !is_nullish(env, argv[0])) ok = get_floats(env, argv[0], rot, 4);
    if (ok && !is_nullish(env, argv[1])) ok = get_floats(env, argv[1], tr, 3);
    if (ok && !is_nullish(env, argv[3])) ok = have_pivot = get_floats(env, argv[3], pv, 3);
    if (!ok) return throw_who(env, napi_throw_type_error, bad.who, bad.what);
    if (!is_nullish(env, argv[2]) && !get_f64(env, argv[2], &scale, &bad)) return NULL;
    gs_xform x;
    int32_t rc = gs_xform_compose(rot, tr, (float)scale, have_pivot ? pv : NULL, &x);
    if (rc != GS_OK) return throw_gs(env, rc);
    return copy_arraybuffer(env, &x, sizeof(x), "composeTransform");
}

/* transformSplats(handle, xform (ArrayBuffer / typed array holding a gs_xform), mask, value) -> matched */
static napi_value js_transform_splats(napi_env env, napi_callback_info info) {
    CTX_ARGS(4, 4);
    static const complaint bad = {"transformSplats", "expects (handle, the buffer composeTransform returned, mask, value)"};
    view xb;
    uint32_t f[2]; /* mask, value */
    if (!get_view(env, argv[1], sizeof(gs_xform), &xb, &bad)) return NULL;
    if (xb.len != sizeof(gs_xform)) return throw_who(env, napi_throw_type_error, bad.who, bad.what);
    if (!get_u32s(env, argv, 2, 2, f, &bad)) return NULL;
    gs_xform x;
    memcpy(&x, xb.data, sizeof(x)); /* (a view may be unaligned) */
    uint64_t matched = 0;
    return ret_u64(env, gs_transform_splats(ctx, f[0], f[1], &x, &matched), &matched);
}

/* setOption(handle, key, value) */
static napi_value js_set_option(napi_env env, napi_callback_info info) {
    CTX_ARGS(3, 3);
    uint32_t key = 0;
    double value = 0;
    if (!get_u32s(env, argv, 1, 1, &key, NULL) || !get_f64(env, argv[2], &value, NULL)) return NULL;
    return ret_none(env, gs_set_option(ctx, (int32_t)key, (int64_t)value));
}

/* stats(handle) -> {numGaussians, numVisible, numIntersections, numProcessed, numTiles, sortPasses, frames, stageUs:[6], frameUs, ...} */
static napi_value js_stats(napi_env env, napi_callback_info info) {
    CTX_ARGS(1, 1);
    gs_stats st;
    int32_t rc = gs_get_stats(ctx, &st);
    if (rc != GS_OK) return throw_gs(env, rc);
    const num_row rows[] = {
        {"numGaussians", (double)st.num_gaussians},   {"numVisible", (double)st.num_visible},
        {"numIntersections", (double)st.num_intersections}, {"numProcessed", (double)st.num_processed},
        {"numTiles", (double)st.num_tiles},           {"sortPasses", (double)st.sort_passes},
        {"frames", (double)st.frames},                {"frameUs", (double)st.frame_us},
        {"numEvaluated", (double)st.num_evaluated},   {"depthOrdered", (double)st.depth_ordered},
        {"tightBinning", (double)st.tight_binning},   {"graphFrames", (double)st.graph_frames},
        {"capacity", (double)st.capacity},            {"maxIntersectionsSeen", (double)st.max_intersections_seen},
        {"truncatedFrames", (double)st.truncated_frames},
    };
    double stage_us[GS_STAGE_COUNT];
    for (uint32_t i = 0; i < GS_STAGE_COUNT; ++i) stage_us[i] = (double)st.stage_us[i];
    return with_prop(env, num_object(env, ROWS(rows)), "stageUs", num_array(env, stage_us, GS_STAGE_COUNT));
}

/* slab(handle) -> {begin, width}: the tile columns this context renders, in pixels */
static napi_value js_slab(napi_env env, napi_callback_info info) {
    CTX_ARGS(1, 1);
    uint32_t b = 0, w = 0;
    int32_t rc = gs_slab_width(ctx, &b, &w);
    if (rc != GS_OK) return throw_gs(env, rc);
    const num_row rows[] = {{"begin", b}, {"width", w}};
    return num_object(env, ROWS(rows));
}

/* loadPly(path) -> {n, degree, records: ArrayBuffer}: the native PackedGaussians (gs_ply_load) */
static napi_value js_load_ply(napi_env env, napi_callback_info info) {
    ARGS(1);
    static const complaint bad = {"loadPly", "path required"};
    char path[GS_PATH_MAX];
    if (!get_path(env, argv[0], path, &bad)) return NULL;
    void* rec = NULL;
    uint64_t n = 0;
    int32_t degree = 0;
    int32_t rc = gs_ply_load(path, &rec, &n, &degree);
    if (rc != GS_OK) return throw_gs(env, rc);
    napi_value ab = copy_arraybuffer(env, rec, (size_t)n * GS_SPLAT_RECORD_BYTES, "loadPly");
    gs_ply_free(rec);
    const num_row rows[] = {{"n", (double)n}, {"degree", (double)degree}};
    return ab ? with_prop(env, num_object(env, ROWS(rows)), "records", ab) : NULL;
}

/* uploadPly(handle, path) -> n : the streaming loader (file -> pinned chunks -> device scene arrays, gs_upload_ply) */
static napi_value js_upload_ply(napi_env env, napi_callback_info info) {
    CTX_ARGS(2, 2);
    static const complaint bad = {"uploadPly", "path required"};
    char path[GS_PATH_MAX];
    if (!get_path(env, argv[1], path, &bad)) return NULL;
    uint64_t n = 0;
    return ret_u64(env, gs_upload_ply(ctx, path, &n), &n);
}

/* hostAlloc(bytes) -> ArrayBuffer over page-locked memory (gs_host_alloc): a frame sink renderToSink copies into asynchronously */
static void finalize_pinned(napi_env env, void* data, void* hint) { (void)env; (void)hint; gs_host_free(data); }
static napi_value js_host_alloc(napi_env env, napi_callback_info info) {
    ARGS(1);
    static const complaint bad = {"hostAlloc", "byte count required"};
    double bytes = 0;
    if (!get_f64(env, argv[0], &bytes, &bad)) return NULL;
    if (!(bytes > 0.0) || bytes > 17179869184.0) return throw_who(env, napi_throw_type_error, bad.who, bad.what);
    void* p = NULL;
    int32_t rc = gs_host_alloc((uint64_t)bytes, &p);
    if (rc != GS_OK) return throw_gs(env, rc);
    napi_value ab;
    if (napi_create_external_arraybuffer(env, p, (size_t)bytes, finalize_pinned, NULL, &ab) != napi_ok) {
        gs_host_free(p);
        return throw_who(env, napi_throw_error, "hostAlloc", "napi_create_external_arraybuffer failed");
    }
    return ab;
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
