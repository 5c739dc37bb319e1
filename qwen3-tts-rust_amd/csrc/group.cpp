// group.cpp -- multi-GPU serving behind the C ABI (include/q3tts.h "multi-GPU").
//
// Utterances are independent (own prompt, KV pages, sampler state, decoder state; /root/reference/src/tts/engine.rs:445-656 touches no
// cross-request state), so GPUs are REQUEST-SHARDED: every device holds the full weights, requests go round-robin, and the data path has
// no collective.  The one exchange step is a voice registration: the VoiceFile payload (speaker embedding 2048 f32 = 8 KB, plus reference
// codes / reference-text ids for clone voices; utils/voice_file.rs:5-22) is sent from the device that owns it to all others --
//   * q3tts_group_*: ONE process drives N devices (one engine, one scheduler thread, one decoder thread per device).  Registration uploads
//     the payload to the first device and broadcasts it device-to-device with ncclBroadcast on communicators from ncclCommInitAll (RCCL,
//     xGMI between the GPUs of a node); when librccl cannot be loaded, or the group has one device, or lists a device twice, the copies
//     are hipMemcpyPeerAsync.  Every engine registers the voice from ITS OWN device's copy of the bytes.
//   * q3tts_comm_*: ONE process per GPU (the layout bench.py and the driver's --gpus N runs use): rank 0 creates a 128-byte id, every rank
//     builds its communicator from it (ncclCommInitRank), and q3tts_comm_voice_register is the collective call.
// RCCL is bound at run time (dlopen "librccl.so"), so libq3tts.so has no link-time dependency on it and single-GPU hosts need not have it.
#include "../../include/q3tts.h"
#include "engine.h"
#include <dlfcn.h>
#include <atomic>
#include <cmath>

using namespace q3;

#define Q3_API_BEGIN try {
#define Q3_API_END(failval) } catch (const std::exception& ex) { set_last_error(ex.what()); return failval; } catch (...) { set_last_error("unknown error"); return failval; }

namespace {

// ---- the few RCCL entry points this file uses (public NCCL API; signatures as in rccl.h) ----
struct NcclId { char internal[128]; };
typedef void* ncclComm_t;
struct Rccl {
    void* h = nullptr;
    int (*GetUniqueId)(NcclId*) = nullptr;
    int (*CommInitRank)(ncclComm_t*, int, NcclId, int) = nullptr;
    int (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    int (*CommDestroy)(ncclComm_t) = nullptr;
    int (*Broadcast)(const void*, void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool ok() const { return h != nullptr; }
};
Rccl& rccl() {
    static Rccl r = [] {
        Rccl x;
        if (const char* e = std::getenv("Q3_NO_RCCL")) if (e[0] == '1') return x; // A/B switch: force the peer-copy path
        void* h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!h) h = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_LOCAL);
        if (!h) return x;
        auto sym = [&](const char* n) { return dlsym(h, n); };
        x.GetUniqueId = (int (*)(NcclId*))sym("ncclGetUniqueId");
        x.CommInitRank = (int (*)(ncclComm_t*, int, NcclId, int))sym("ncclCommInitRank");
        x.CommInitAll = (int (*)(ncclComm_t*, int, const int*))sym("ncclCommInitAll");
        x.CommDestroy = (int (*)(ncclComm_t))sym("ncclCommDestroy");
        x.Broadcast = (int (*)(const void*, void*, size_t, int, int, ncclComm_t, hipStream_t))sym("ncclBroadcast");
        x.GroupStart = (int (*)())sym("ncclGroupStart");
        x.GroupEnd = (int (*)())sym("ncclGroupEnd");
        x.GetErrorString = (const char* (*)(int))sym("ncclGetErrorString");
        if (x.GetUniqueId && x.CommInitRank && x.CommInitAll && x.CommDestroy && x.Broadcast && x.GroupStart && x.GroupEnd) x.h = h;
        return x;
    }();
    return r;
}
void nccl_check(int rc, const char* what) {
    if (rc != 0) throw Error(std::string(what) + ": " + (rccl().GetErrorString ? rccl().GetErrorString(rc) : "RCCL error ") + " (" + std::to_string(rc) + ")");
}
constexpr int kNcclChar = 0; // ncclInt8 / ncclChar

// ---- voice payload: header {n_emb, n_codes, n_text, magic} i64 x 4, then f32 embedding, i32 codes, i32 text ids ----
constexpr int64_t kVoiceMagic = 0x5133564F49434531ll; // "Q3VOICE1"
constexpr size_t kHdrBytes = 32;
std::vector<uint8_t> pack_voice(const float* spk, const int32_t* codes, int32_t n_codes, const int32_t* text, int32_t n_text) {
    Q3_CHECK(spk, "speaker embedding missing");
    Q3_CHECK(n_codes >= 0 && n_text >= 0 && (n_codes == 0 || codes) && (n_text == 0 || text), "bad voice arrays");
    const int64_t hdr[4] = {Q3_EMBD, n_codes, n_text, kVoiceMagic};
    std::vector<uint8_t> b(kHdrBytes + (size_t)Q3_EMBD * 4 + (size_t)n_codes * 4 + (size_t)n_text * 4);
    std::memcpy(b.data(), hdr, kHdrBytes);
    std::memcpy(b.data() + kHdrBytes, spk, (size_t)Q3_EMBD * 4);
    if (n_codes) std::memcpy(b.data() + kHdrBytes + (size_t)Q3_EMBD * 4, codes, (size_t)n_codes * 4);
    if (n_text) std::memcpy(b.data() + kHdrBytes + (size_t)Q3_EMBD * 4 + (size_t)n_codes * 4, text, (size_t)n_text * 4);
    return b;
}
size_t payload_bytes(const int64_t hdr[4]) {
    Q3_CHECK(hdr[3] == kVoiceMagic && hdr[0] == Q3_EMBD && hdr[1] >= 0 && hdr[1] <= (1 << 24) && hdr[2] >= 0 && hdr[2] <= (1 << 20), "corrupt voice header");
    return (size_t)hdr[0] * 4 + (size_t)hdr[1] * 4 + (size_t)hdr[2] * 4;
}
Voice unpack_voice(const uint8_t* b) {
    int64_t hdr[4];
    std::memcpy(hdr, b, kHdrBytes);
    (void)payload_bytes(hdr);
    Voice v;
    const float* e = reinterpret_cast<const float*>(b + kHdrBytes);
    v.spk_emb.assign(e, e + hdr[0]);
    const int32_t* c = reinterpret_cast<const int32_t*>(b + kHdrBytes + (size_t)hdr[0] * 4);
    v.ref_codes.assign(c, c + hdr[1]);
    v.ref_text_ids.assign(c + hdr[1], c + hdr[1] + hdr[2]);
    return v;
}

struct DevSlot { // per-device staging for the broadcast
    int dev = 0; hipStream_t st = nullptr; uint8_t* d_buf = nullptr; uint8_t* h_buf = nullptr; size_t cap = 0;
    void ensure(size_t n) {
        if (n <= cap) return;
        Q3_HIP(hipSetDevice(dev));
        if (d_buf) (void)hipFree(d_buf);
        if (h_buf) (void)hipHostFree(h_buf);
        cap = (n + 4095) & ~(size_t)4095;
        Q3_HIP(hipMalloc((void**)&d_buf, cap));
        Q3_HIP(hipHostMalloc((void**)&h_buf, cap));
    }
    void release() {
        (void)hipSetDevice(dev);
        if (d_buf) (void)hipFree(d_buf);
        if (h_buf) (void)hipHostFree(h_buf);
        if (st) (void)hipStreamDestroy(st);
        d_buf = h_buf = nullptr; st = nullptr; cap = 0;
    }
};

} // namespace

struct q3tts_engine; // defined in capi.cpp
extern "C" {
int q3tts_engine_create(const q3tts_engine_params* p, q3tts_engine** out);
void q3tts_engine_destroy(q3tts_engine* e);
}

struct q3tts_group {
    std::vector<q3tts_engine*> eng;
    std::vector<DevSlot> slot;
    std::vector<ncclComm_t> comm; // empty => peer copies
    std::atomic<uint64_t> rr{0};
    std::mutex mu; // serialises registrations
    bool started = false;
    bool distinct = true;                 // every listed device is a different one
    int64_t n_reg_rccl = 0, n_reg_peer = 0; // registrations by the path their bytes took (q3tts_group_info)
    bool path_logged = false;
    ~q3tts_group() {
        for (auto c : comm) if (c) (void)rccl().CommDestroy(c);
        for (auto& s : slot) s.release();
        for (auto* e : eng) if (e) q3tts_engine_destroy(e);
    }
};
struct q3tts_comm {
    ncclComm_t comm = nullptr; int rank = 0, world = 1; DevSlot slot;
    ~q3tts_comm() { if (comm) (void)rccl().CommDestroy(comm); slot.release(); }
};

static const int kEngineBits = 8; // group request id = (engine request id << 8) | engine index
static inline int eng_of(int64_t id) { return (int)(id & ((1 << kEngineBits) - 1)); }
static inline int64_t rid_of(int64_t id) { return id >> kEngineBits; }

extern "C" {

int q3tts_group_create(const q3tts_engine_params* p, const int32_t* device_ids, int32_t n_dev, q3tts_group** out) {
    Q3_API_BEGIN
    Q3_CHECK(p && out && device_ids && n_dev >= 1 && n_dev <= (1 << kEngineBits), "bad arguments");
    int n_vis = 0;
    if (hipGetDeviceCount(&n_vis) != hipSuccess || n_vis <= 0) throw Error("no HIP device available: the HIP path is the only compute path (no CPU fallback)");
    bool distinct = true;
    for (int i = 0; i < n_dev; i++) {
        Q3_CHECK(device_ids[i] >= 0 && device_ids[i] < n_vis, "device id out of range");
        for (int j = 0; j < i; j++) if (device_ids[j] == device_ids[i]) distinct = false;
    }
    std::unique_ptr<q3tts_group> g(new q3tts_group());
    g->distinct = distinct;
    g->eng.assign(n_dev, nullptr);
    g->slot.resize(n_dev);
    for (int i = 0; i < n_dev; i++) {
        q3tts_engine_params pi = *p;
        pi.device = device_ids[i];
        if (q3tts_engine_create(&pi, &g->eng[i]) != Q3TTS_OK) throw Error(std::string("engine on device ") + std::to_string(device_ids[i]) + ": " + last_error());
        g->slot[i].dev = device_ids[i];
        Q3_HIP(hipSetDevice(device_ids[i]));
        Q3_HIP(hipStreamCreateWithFlags(&g->slot[i].st, hipStreamNonBlocking));
        for (int j = 0; j < i; j++) { // peer access for the copy path (and for RCCL's direct xGMI transport)
            int can = 0;
            if (device_ids[j] != device_ids[i] && hipDeviceCanAccessPeer(&can, device_ids[i], device_ids[j]) == hipSuccess && can) {
                (void)hipDeviceEnablePeerAccess(device_ids[j], 0); (void)hipGetLastError();
                (void)hipSetDevice(device_ids[j]); (void)hipDeviceEnablePeerAccess(device_ids[i], 0); (void)hipGetLastError();
                (void)hipSetDevice(device_ids[i]);
            }
        }
    }
    if (n_dev > 1 && distinct && rccl().ok()) {
        g->comm.assign(n_dev, nullptr);
        std::vector<int> devs(device_ids, device_ids + n_dev);
        nccl_check(rccl().CommInitAll(g->comm.data(), n_dev, devs.data()), "ncclCommInitAll");
    }
    *out = g.release();
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
void q3tts_group_destroy(q3tts_group* g) { delete g; }
int32_t q3tts_group_size(q3tts_group* g) { return g ? (int32_t)g->eng.size() : 0; }
q3tts_engine* q3tts_group_engine(q3tts_group* g, int32_t i) { return (g && i >= 0 && i < (int)g->eng.size()) ? g->eng[i] : nullptr; }
int32_t q3tts_group_uses_rccl(q3tts_group* g) { return g && !g->comm.empty() ? 1 : 0; }
int q3tts_group_info(q3tts_group* g, q3tts_group_info_t* out) {
    Q3_API_BEGIN
    Q3_CHECK(g && out, "null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    out->n_devices = (int32_t)g->eng.size();
    out->rccl_loaded = rccl().ok() ? 1 : 0;
    out->rccl_ranks = (int32_t)g->comm.size();
    out->distinct_devices = g->distinct ? 1 : 0;
    out->registrations_rccl = g->n_reg_rccl;
    out->registrations_peer_copy = g->n_reg_peer;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

int q3tts_group_voice_register(q3tts_group* g, const float* spk, const int32_t* ref_codes, int32_t n_ref_codes, const int32_t* ref_text,
                               int32_t n_ref_text, int32_t* voice_id) {
    Q3_API_BEGIN
    Q3_CHECK(g && spk && voice_id, "null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    const std::vector<uint8_t> pay = pack_voice(spk, ref_codes, n_ref_codes, ref_text, n_ref_text);
    const int n = (int)g->eng.size();
    { std::lock_guard<std::mutex> cap(capture_mutex()); for (auto& s : g->slot) s.ensure(pay.size()); } // allocations never overlap a running engine's capture
    // the owner (first device) uploads once ...
    DevSlot& s0 = g->slot[0];
    Q3_HIP(hipSetDevice(s0.dev));
    std::memcpy(s0.h_buf, pay.data(), pay.size());
    Q3_HIP(hipMemcpyAsync(s0.d_buf, s0.h_buf, pay.size(), hipMemcpyHostToDevice, s0.st));
    Q3_HIP(hipStreamSynchronize(s0.st));
    // ... and the bytes travel device to device
    if (!g->path_logged) { // once per group: which path registrations take (a multi-GPU run must be able to show "RCCL, N ranks", not assume it)
        g->path_logged = true;
        std::fprintf(stderr, "[q3tts group] voice registrations: %s over %d device(s)%s\n", !g->comm.empty() ? "ncclBroadcast (RCCL communicators from ncclCommInitAll)" :
                     n > 1 ? "hipMemcpyPeerAsync (no RCCL communicators)" : "single device, no exchange", n,
                     g->comm.empty() && n > 1 ? (!g->distinct ? " -- a device is listed twice" : !rccl().ok() ? " -- librccl not loaded" : "") : "");
    }
    if (!g->comm.empty()) g->n_reg_rccl++; else if (n > 1) g->n_reg_peer++;
    if (!g->comm.empty()) {
        nccl_check(rccl().GroupStart(), "ncclGroupStart");
        for (int i = 0; i < n; i++) {
            Q3_HIP(hipSetDevice(g->slot[i].dev));
            nccl_check(rccl().Broadcast(g->slot[i].d_buf, g->slot[i].d_buf, pay.size(), kNcclChar, 0, g->comm[i], g->slot[i].st), "ncclBroadcast");
        }
        nccl_check(rccl().GroupEnd(), "ncclGroupEnd");
    } else {
        for (int i = 1; i < n; i++) {
            Q3_HIP(hipSetDevice(g->slot[i].dev));
            Q3_HIP(hipMemcpyPeerAsync(g->slot[i].d_buf, g->slot[i].dev, s0.d_buf, s0.dev, pay.size(), g->slot[i].st));
        }
    }
    int vid = -1;
    for (int i = 0; i < n; i++) { // every engine registers from its own device's copy
        DevSlot& s = g->slot[i];
        Q3_HIP(hipSetDevice(s.dev));
        if (i > 0) std::memset(s.h_buf, 0, pay.size());
        Q3_HIP(hipMemcpyAsync(s.h_buf, s.d_buf, pay.size(), hipMemcpyDeviceToHost, s.st));
        Q3_HIP(hipStreamSynchronize(s.st));
        const Voice v = unpack_voice(s.h_buf);
        int32_t id = -1;
        if (q3tts_voice_register(g->eng[i], v.spk_emb.data(), v.ref_codes.empty() ? nullptr : v.ref_codes.data(), (int32_t)v.ref_codes.size(),
                                 v.ref_text_ids.empty() ? nullptr : v.ref_text_ids.data(), (int32_t)v.ref_text_ids.size(), &id) != Q3TTS_OK)
            throw Error(std::string("voice registration on engine ") + std::to_string(i) + ": " + last_error());
        if (i == 0) vid = id;
        Q3_CHECK(id == vid, "engines of a group must hand out the same voice ids (register voices through the group only)");
    }
    *voice_id = vid;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

// ---- the forwarders: every function from here to q3tts_group_stop is one of four shapes, each written once ----
} // extern "C"
namespace {
// 1. by request id: fn(the engine the id names, the engine's own id, a...)
template <class F, class... A> int routed(q3tts_group* g, int64_t id, F fn, A... a) {
    if (!g || eng_of(id) >= (int)g->eng.size()) { set_last_error("unknown group request id"); return Q3TTS_ERR; }
    return fn(g->eng[eng_of(id)], rid_of(id), a...);
}
// 2. a submission on one engine: engine_index, or the next in turn (kNext; SURVEY 8e: request i -> device i % n).  call(engine) leaves n engine
// ids in ids, which come back tagged with the engine's index; a refused submission still takes its turn
constexpr int32_t kNext = -1;
template <class F> int submit_on(q3tts_group* g, bool have_args, int32_t engine_index, int64_t* ids, int n, F call) {
    Q3_API_BEGIN
    Q3_CHECK(have_args, "null argument");
    Q3_CHECK(engine_index >= kNext && engine_index < (int)g->eng.size(), "engine_index outside the group (-1 = round robin)");
    const int i = engine_index >= 0 ? engine_index : (int)(g->rr.fetch_add(1) % g->eng.size());
    if (call(g->eng[i]) != Q3TTS_OK) return Q3TTS_ERR;
    for (int k = 0; k < n; k++) ids[k] = (ids[k] << kEngineBits) | i;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
// 3. on every engine.  ALL_OR_STOP: the first failure ends the walk (the engines are alike: what one refuses the others would); EVERY: each
// engine is called whatever the others said, and one failure makes the answer (a release, a stop).  null_msg = null: a null group fails silently
enum Walk { ALL_OR_STOP, EVERY };
template <class F> int on_every(q3tts_group* g, Walk walk, F call, const char* null_msg = "null argument") {
    if (!g) { if (null_msg) set_last_error(null_msg); return Q3TTS_ERR; }
    int rc = Q3TTS_OK;
    for (auto* e : g->eng) if (call(e) != Q3TTS_OK) { rc = Q3TTS_ERR; if (walk == ALL_OR_STOP) break; }
    return rc;
}
// 4. held objects ([EXT] codec preambles, prompt stems): built on every engine under one id, as voices are.  The engines of a group are alike
// and hand out ids in order, so what the first engine accepts the others accept under the same id; one created on a single engine behind
// the group's back breaks that
struct HeldCalls {
    const char* noun;
    int (*poll)(q3tts_engine*, int32_t, int32_t*, int32_t*); int (*wait)(q3tts_engine*, int32_t, double); int (*release)(q3tts_engine*, int32_t);
    int (*set_voice)(q3tts_engine*, int32_t, int32_t); int (*set_engine)(q3tts_engine*, int32_t);
};
const HeldCalls kPreamble = {"preamble", q3tts_preamble_poll, q3tts_preamble_wait, q3tts_preamble_release, q3tts_voice_set_preamble, q3tts_engine_set_preamble};
const HeldCalls kStem = {"stem", q3tts_stem_poll, q3tts_stem_wait, q3tts_stem_release, q3tts_voice_set_stem, q3tts_engine_set_stem};
template <class F> int held_create(q3tts_group* g, const HeldCalls& k, int32_t* id_out, F create) {
    Q3_API_BEGIN
    Q3_CHECK(g && id_out, "null argument");
    int32_t first = -1;
    for (size_t i = 0; i < g->eng.size(); i++) {
        int32_t id = -1;
        if (create(g->eng[i], &id) != Q3TTS_OK) {
            const std::string why = last_error();
            for (size_t j = 0; j < i; j++) (void)k.release(g->eng[j], first); // all engines or none
            throw Error(why);
        }
        if (i == 0) first = id;
        Q3_CHECK(id == first, std::string("engines of a group must hand out the same ") + k.noun + " ids (create " + k.noun + "s through the group only)");
    }
    *id_out = first;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int held_wait(q3tts_group* g, const HeldCalls& k, int32_t id, double timeout_ms) { // 0 once every engine's copy is READY or FAILED, 1 on timeout
    if (!g) { set_last_error("null argument"); return Q3TTS_ERR; }
    int worst = 0;
    for (auto* e : g->eng) {
        const int rc = k.wait(e, id, timeout_ms);
        if (rc < 0) return rc;
        worst = std::max(worst, rc);
    }
    return worst;
}
// a setter takes an object that is READY on every engine, checked before any engine is touched: all engines or none
template <class F> int held_set(q3tts_group* g, const HeldCalls& k, int32_t id, F set) {
    if (!g) { set_last_error("null argument"); return Q3TTS_ERR; }
    const HeldWords words(k.noun); // owns the text set_refusal points into
    for (size_t i = 0; id >= 0 && i < g->eng.size(); i++) {
        int32_t st = 0;
        if (k.poll(g->eng[i], id, &st, nullptr) != Q3TTS_OK) return Q3TTS_ERR;
        if (const char* why = words.set_refusal(true, st)) { set_last_error(why); return Q3TTS_ERR; }
    }
    return on_every(g, ALL_OR_STOP, set);
}
} // namespace
extern "C" {

int q3tts_group_submit(q3tts_group* g, const q3tts_request* r, int32_t want_pcm, int64_t* req_id) { return q3tts_group_submit_ex(g, r, want_pcm, nullptr, req_id); }
int q3tts_group_submit_ex(q3tts_group* g, const q3tts_request* r, int32_t want_pcm, const q3tts_gen_options* opts, int64_t* req_id) {
    return submit_on(g, g && r && req_id, kNext, req_id, 1, [&](q3tts_engine* e) { return q3tts_submit_ex(e, r, want_pcm, opts, req_id); });
}
int q3tts_group_submit_text(q3tts_group* g, int32_t voice_id, const int32_t* text_ids, int32_t n_text, int32_t lang_id, const int32_t* instr_ids,
                            int32_t n_instr, const q3tts_sampler_config* sampler, int32_t max_steps, int32_t mask_eos, int32_t want_pcm, int64_t* req_id) {
    return q3tts_group_submit_text_ex(g, voice_id, text_ids, n_text, lang_id, instr_ids, n_instr, sampler, max_steps, mask_eos, want_pcm, nullptr, req_id);
}
int q3tts_group_submit_text_ex(q3tts_group* g, int32_t voice_id, const int32_t* text_ids, int32_t n_text, int32_t lang_id, const int32_t* instr_ids,
                               int32_t n_instr, const q3tts_sampler_config* sampler, int32_t max_steps, int32_t mask_eos, int32_t want_pcm,
                               const q3tts_gen_options* opts, int64_t* req_id) {
    return submit_on(g, g && req_id, kNext, req_id, 1, [&](q3tts_engine* e) {
        return q3tts_submit_text_ex(e, voice_id, text_ids, n_text, lang_id, instr_ids, n_instr, sampler, max_steps, mask_eos, want_pcm, opts, req_id); });
}
int q3tts_group_submit_text_streaming(q3tts_group* g, int32_t voice_id, const int32_t* text_ids, int32_t n_text, int32_t lang_id,
                                      const int32_t* instr_ids, int32_t n_instr, const q3tts_sampler_config* sampler, int32_t max_steps,
                                      int32_t mask_eos, int32_t want_pcm, const q3tts_gen_options* opts, int64_t* req_id) {
    return submit_on(g, g && req_id, kNext, req_id, 1, [&](q3tts_engine* e) {
        return q3tts_submit_text_streaming(e, voice_id, text_ids, n_text, lang_id, instr_ids, n_instr, sampler, max_steps, mask_eos, want_pcm, opts, req_id); });
}
int q3tts_group_submit_text_streaming_open(q3tts_group* g, int32_t voice_id, const int32_t* text_ids, int32_t n_text, int32_t lang_id,
                                           const int32_t* instr_ids, int32_t n_instr, const q3tts_sampler_config* sampler,
                                           int32_t max_steps, int32_t mask_eos, int32_t want_pcm, const q3tts_gen_options* opts,
                                           int64_t* req_id) {
    return submit_on(g, g && req_id, kNext, req_id, 1, [&](q3tts_engine* e) {
        return q3tts_submit_text_streaming_open(e, voice_id, text_ids, n_text, lang_id, instr_ids, n_instr, sampler, max_steps, mask_eos, want_pcm, opts, req_id); });
}
int q3tts_group_submit_resume(q3tts_group* g, int32_t engine_index, const q3tts_request* r, int32_t want_pcm, const q3tts_gen_options* opts,
                              const int32_t* trail_ids, int32_t n_trail, int32_t open, const int32_t* prefix_codes, int32_t n_prefix, int64_t* req_id) {
    return submit_on(g, g && r && req_id, engine_index, req_id, 1, [&](q3tts_engine* e) {
        return q3tts_submit_resume(e, r, want_pcm, opts, trail_ids, n_trail, open, prefix_codes, n_prefix, req_id); });
}
int q3tts_group_submit_score(q3tts_group* g, int32_t engine_index, const float* prompt, int32_t n_prompt, const int32_t* trail_ids, int32_t n_trail,
                             const int32_t* codes, int32_t n, int64_t* req_id) {
    return submit_on(g, g && req_id, engine_index, req_id, 1, [&](q3tts_engine* e) { return q3tts_submit_score(e, prompt, n_prompt, trail_ids, n_trail, codes, n, req_id); });
}
int q3tts_group_submit_decode(q3tts_group* g, int32_t engine_index, const int32_t* codes, int32_t n, int64_t* req_id) {
    return submit_on(g, g && codes && req_id, engine_index, req_id, 1, [&](q3tts_engine* e) { return q3tts_submit_decode(e, codes, n, req_id); });
}
int q3tts_group_submit_candidates(q3tts_group* g, int32_t engine_index, const q3tts_request* r, int32_t want_pcm, const q3tts_gen_options* opts,
                                  const int32_t* trail_ids, int32_t n_trail, const uint64_t* seeds, int32_t n, int64_t* req_ids) {
    return submit_on(g, g && r, engine_index, req_ids, n, [&](q3tts_engine* e) { // req_ids: the engine's own check
        return q3tts_submit_candidates(e, r, want_pcm, opts, trail_ids, n_trail, seeds, n, req_ids); });
}

int32_t q3tts_group_device_of(q3tts_group* g, int64_t req_id) { return (g && eng_of(req_id) < (int)g->slot.size()) ? g->slot[eng_of(req_id)].dev : -1; }
int q3tts_group_text_append(q3tts_group* g, int64_t req_id, const int32_t* text_ids, int32_t n, int32_t is_last) { return routed(g, req_id, q3tts_text_append, text_ids, n, is_last); }
int q3tts_group_trail_append(q3tts_group* g, int64_t req_id, const int32_t* ids, int32_t n, int32_t close) { return routed(g, req_id, q3tts_trail_append, ids, n, close); }
int q3tts_group_trail_progress(q3tts_group* g, int64_t req_id, int32_t* n_appended, int32_t* n_consumed, int32_t* closed) {
    return routed(g, req_id, q3tts_trail_progress, n_appended, n_consumed, closed);
}
int q3tts_group_poll(q3tts_group* g, int64_t req_id, q3tts_req_status* out) { return routed(g, req_id, q3tts_poll, out); }
int q3tts_group_fetch(q3tts_group* g, int64_t req_id, int32_t* codes_out, int32_t frame_off, int32_t max_frames, float* pcm_out, int64_t pcm_off,
                      int64_t pcm_cap, int32_t* got_frames, int64_t* got_pcm) {
    return routed(g, req_id, q3tts_fetch, codes_out, frame_off, max_frames, pcm_out, pcm_off, pcm_cap, got_frames, got_pcm);
}
int q3tts_group_wait(q3tts_group* g, int64_t req_id, double timeout_ms) { return routed(g, req_id, q3tts_wait, timeout_ms); }
int q3tts_group_release(q3tts_group* g, int64_t req_id) { return routed(g, req_id, q3tts_release); }
int q3tts_group_cancel(q3tts_group* g, int64_t req_id) { return routed(g, req_id, q3tts_cancel); }
int q3tts_group_fetch_logprobs(q3tts_group* g, int64_t req_id, float* out, int32_t frame_off, int32_t max_frames, int32_t* got_frames) {
    return routed(g, req_id, q3tts_fetch_logprobs, out, frame_off, max_frames, got_frames);
}
int q3tts_group_fetch_pcm16(q3tts_group* g, int64_t req_id, int16_t* out, int64_t off, int64_t cap, int64_t* got) { return routed(g, req_id, q3tts_fetch_pcm16, out, off, cap, got); }
int q3tts_group_request_format(q3tts_group* g, int64_t req_id, q3tts_pcm_format* out) { return routed(g, req_id, q3tts_request_format, out); }
int q3tts_group_request_preamble(q3tts_group* g, int64_t req_id, int32_t* preamble_id) { return routed(g, req_id, q3tts_request_preamble, preamble_id); }
int q3tts_group_request_stem(q3tts_group* g, int64_t req_id, int32_t* stem_id, int32_t* rows_reused) { return routed(g, req_id, q3tts_request_stem, stem_id, rows_reused); }
int q3tts_group_request_speech_rate(q3tts_group* g, int64_t req_id, int32_t* rate_pct) { return routed(g, req_id, q3tts_request_speech_rate, rate_pct); }

// [EXT] the engine-level settings, on every engine; a value is checked before any engine is touched: all engines or none
int q3tts_group_set_logprobs(q3tts_group* g, int32_t on) { return on_every(g, ALL_OR_STOP, [&](q3tts_engine* e) { return q3tts_engine_set_logprobs(e, on); }); }
int q3tts_group_set_output_format(q3tts_group* g, const q3tts_pcm_format* f) {
    if (g && f && q3tts_pcm_format_check(f) != Q3TTS_OK) return Q3TTS_ERR;
    return on_every(g, ALL_OR_STOP, [&](q3tts_engine* e) { return q3tts_engine_set_output_format(e, f); });
}
int q3tts_group_request_pitch(q3tts_group* g, int64_t req_id, int32_t* pitch_pct) { return routed(g, req_id, q3tts_request_pitch, pitch_pct); }
int q3tts_group_set_pitch(q3tts_group* g, int32_t pitch_pct) { // [EXT] q3tts_engine_set_pitch on every engine: all of them or none
    if (g && q3tts_pitch_plan(pitch_pct, nullptr, nullptr, nullptr, nullptr) != Q3TTS_OK) { set_last_error("pitch out of range [50, 200]"); return Q3TTS_ERR; }
    return on_every(g, ALL_OR_STOP, [&](q3tts_engine* e) { return q3tts_engine_set_pitch(e, pitch_pct); });
}
int q3tts_group_request_volume(q3tts_group* g, int64_t req_id, int32_t* db10) { return routed(g, req_id, q3tts_request_volume, db10); }
int q3tts_group_set_volume(q3tts_group* g, int32_t db10) { // [EXT] q3tts_engine_set_volume on every engine: all of them or none
    if (g && std::isnan(q3tts_volume_gain(db10))) { set_last_error("volume out of range [-400, 200]"); return Q3TTS_ERR; }
    return on_every(g, ALL_OR_STOP, [&](q3tts_engine* e) { return q3tts_engine_set_volume(e, db10); });
}
// [EXT] loudness: the meter on every engine, and a request's rows and summary from the engine that runs it
int q3tts_group_set_loudness(q3tts_group* g, int32_t on) { return on_every(g, ALL_OR_STOP, [&](q3tts_engine* e) { return q3tts_engine_set_loudness(e, on); }); }
int q3tts_group_fetch_loudness(q3tts_group* g, int64_t req_id, double* out, int64_t block_off, int64_t max_blocks, int64_t* got) {
    return routed(g, req_id, q3tts_fetch_loudness, out, block_off, max_blocks, got);
}
int q3tts_group_request_loudness(q3tts_group* g, int64_t req_id, q3tts_loudness* out) { return routed(g, req_id, q3tts_request_loudness, out); }
int q3tts_group_request_metered(q3tts_group* g, int64_t req_id, int32_t* on) { return routed(g, req_id, q3tts_request_metered, on); }
int q3tts_group_set_speech_rate(q3tts_group* g, int32_t rate_pct) {
    if (g && q3tts_tsm_samples(rate_pct, 0, 0) < 0) { set_last_error("speech rate out of range [50, 200]"); return Q3TTS_ERR; }
    return on_every(g, ALL_OR_STOP, [&](q3tts_engine* e) { return q3tts_engine_set_speech_rate(e, rate_pct); });
}
int q3tts_group_start(q3tts_group* g) { // one scheduler thread per device
    const int rc = on_every(g, ALL_OR_STOP, q3tts_sched_start, nullptr);
    if (rc == Q3TTS_OK) g->started = true;
    return rc;
}
int q3tts_group_stop(q3tts_group* g) {
    const int rc = on_every(g, EVERY, q3tts_sched_stop, nullptr);
    if (g) g->started = false;
    return rc;
}

// [EXT] codec preambles
int q3tts_group_preamble_create(q3tts_group* g, const int32_t* codes, int32_t n, int32_t* preamble_id) {
    return held_create(g, kPreamble, preamble_id, [&](q3tts_engine* e, int32_t* id) { return q3tts_preamble_create(e, codes, n, id); });
}
int q3tts_group_preamble_wait(q3tts_group* g, int32_t preamble_id, double timeout_ms) { return held_wait(g, kPreamble, preamble_id, timeout_ms); }
int q3tts_group_preamble_release(q3tts_group* g, int32_t preamble_id) { return on_every(g, EVERY, [&](q3tts_engine* e) { return q3tts_preamble_release(e, preamble_id); }); }
int q3tts_group_voice_set_preamble(q3tts_group* g, int32_t voice_id, int32_t preamble_id) {
    return held_set(g, kPreamble, preamble_id, [&](q3tts_engine* e) { return q3tts_voice_set_preamble(e, voice_id, preamble_id); });
}
int q3tts_group_set_preamble(q3tts_group* g, int32_t preamble_id) {
    return held_set(g, kPreamble, preamble_id, [&](q3tts_engine* e) { return q3tts_engine_set_preamble(e, preamble_id); });
}
// [EXT] prompt stems
int q3tts_group_stem_create(q3tts_group* g, const float* rows, int32_t n_rows, int32_t* stem_id) {
    return held_create(g, kStem, stem_id, [&](q3tts_engine* e, int32_t* id) { return q3tts_stem_create(e, rows, n_rows, id); });
}
int q3tts_group_voice_stem_create(q3tts_group* g, int32_t voice_id, int32_t lang_id, const int32_t* instr_ids, int32_t n_instr, int32_t* stem_id) {
    return held_create(g, kStem, stem_id, [&](q3tts_engine* e, int32_t* id) { return q3tts_voice_stem_create(e, voice_id, lang_id, instr_ids, n_instr, id); });
}
int q3tts_group_stem_wait(q3tts_group* g, int32_t stem_id, double timeout_ms) { return held_wait(g, kStem, stem_id, timeout_ms); }
int q3tts_group_stem_release(q3tts_group* g, int32_t stem_id) { return on_every(g, EVERY, [&](q3tts_engine* e) { return q3tts_stem_release(e, stem_id); }); }
int q3tts_group_voice_set_stem(q3tts_group* g, int32_t voice_id, int32_t stem_id) {
    return held_set(g, kStem, stem_id, [&](q3tts_engine* e) { return q3tts_voice_set_stem(e, voice_id, stem_id); });
}
int q3tts_group_set_stem(q3tts_group* g, int32_t stem_id) {
    return held_set(g, kStem, stem_id, [&](q3tts_engine* e) { return q3tts_engine_set_stem(e, stem_id); });
}
int q3tts_group_stem_stats(q3tts_group* g, q3tts_stem_stats* out) { // the engines' counters added up
    if (!g || !out) { set_last_error("null argument"); return Q3TTS_ERR; }
    q3tts_stem_stats sum = {0, 0, 0, 0, 0, 0};
    for (auto* e : g->eng) {
        q3tts_stem_stats s;
        if (q3tts_engine_stem_stats(e, &s) != Q3TTS_OK) return Q3TTS_ERR;
        sum.built += s.built; sum.restores += s.restores; sum.rows_not_prefilled += s.rows_not_prefilled; sum.pages_copied += s.pages_copied;
        sum.mismatches += s.mismatches; sum.device_bytes += s.device_bytes;
    }
    *out = sum;
    return Q3TTS_OK;
}

// ---------------- one process per GPU ----------------
int q3tts_comm_available(void) { return rccl().ok() ? 1 : 0; }
int q3tts_comm_unique_id(uint8_t out[128]) {
    Q3_API_BEGIN
    Q3_CHECK(out, "null argument");
    if (!rccl().ok()) throw Error("librccl.so could not be loaded");
    NcclId id;
    nccl_check(rccl().GetUniqueId(&id), "ncclGetUniqueId");
    std::memcpy(out, id.internal, 128);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_comm_create(const uint8_t id[128], int32_t rank, int32_t world, int32_t device, q3tts_comm** out) {
    Q3_API_BEGIN
    Q3_CHECK(id && out && world >= 1 && rank >= 0 && rank < world, "bad arguments");
    if (!rccl().ok()) throw Error("librccl.so could not be loaded");
    std::unique_ptr<q3tts_comm> c(new q3tts_comm());
    c->rank = rank; c->world = world; c->slot.dev = device;
    Q3_HIP(hipSetDevice(device));
    Q3_HIP(hipStreamCreateWithFlags(&c->slot.st, hipStreamNonBlocking));
    NcclId nid;
    std::memcpy(nid.internal, id, 128);
    nccl_check(rccl().CommInitRank(&c->comm, world, nid, rank), "ncclCommInitRank");
    *out = c.release();
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
void q3tts_comm_destroy(q3tts_comm* c) { delete c; }
int q3tts_comm_voice_register(q3tts_comm* c, q3tts_engine* e, int32_t root, const float* spk, const int32_t* ref_codes, int32_t n_ref_codes,
                              const int32_t* ref_text, int32_t n_ref_text, int32_t* voice_id) {
    Q3_API_BEGIN
    Q3_CHECK(c && e && voice_id && root >= 0 && root < c->world, "bad arguments");
    DevSlot& s = c->slot;
    Q3_HIP(hipSetDevice(s.dev));
    std::vector<uint8_t> pay;
    if (c->rank == root) pay = pack_voice(spk, ref_codes, n_ref_codes, ref_text, n_ref_text);
    // 1) the 32-byte header (sizes are known at the root only), 2) the payload
    { std::lock_guard<std::mutex> cap(capture_mutex()); s.ensure(kHdrBytes); }
    if (c->rank == root) { std::memcpy(s.h_buf, pay.data(), kHdrBytes); Q3_HIP(hipMemcpyAsync(s.d_buf, s.h_buf, kHdrBytes, hipMemcpyHostToDevice, s.st)); }
    nccl_check(rccl().Broadcast(s.d_buf, s.d_buf, kHdrBytes, kNcclChar, root, c->comm, s.st), "ncclBroadcast(header)");
    Q3_HIP(hipMemcpyAsync(s.h_buf, s.d_buf, kHdrBytes, hipMemcpyDeviceToHost, s.st));
    Q3_HIP(hipStreamSynchronize(s.st));
    int64_t hdr[4];
    std::memcpy(hdr, s.h_buf, kHdrBytes);
    const size_t total = kHdrBytes + payload_bytes(hdr);
    { std::lock_guard<std::mutex> cap(capture_mutex()); s.ensure(total); }
    if (c->rank == root) { std::memcpy(s.h_buf, pay.data(), total); Q3_HIP(hipMemcpyAsync(s.d_buf, s.h_buf, total, hipMemcpyHostToDevice, s.st)); }
    nccl_check(rccl().Broadcast(s.d_buf, s.d_buf, total, kNcclChar, root, c->comm, s.st), "ncclBroadcast(voice)");
    if (c->rank != root) std::memset(s.h_buf, 0, total);
    Q3_HIP(hipMemcpyAsync(s.h_buf, s.d_buf, total, hipMemcpyDeviceToHost, s.st));
    Q3_HIP(hipStreamSynchronize(s.st));
    const Voice v = unpack_voice(s.h_buf);
    return q3tts_voice_register(e, v.spk_emb.data(), v.ref_codes.empty() ? nullptr : v.ref_codes.data(), (int32_t)v.ref_codes.size(),
                                v.ref_text_ids.empty() ? nullptr : v.ref_text_ids.data(), (int32_t)v.ref_text_ids.size(), voice_id);
    Q3_API_END(Q3TTS_ERR)
}

} // extern "C"
