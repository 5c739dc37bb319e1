// out_chain.cpp -- see out_chain.h
#include "out_chain.h"

namespace q3 {

OutChain::OutChain(int n_streams, int gmax, int n_lanes, size_t lane_floats)
    : n_streams_(n_streams), gmax_(gmax), n_lanes_(n_lanes), lane_floats_(lane_floats), prosody_((size_t)n_streams) {
    const std::vector<int64_t> z((size_t)gmax, 0);
    for (int l = 0; l < n_lanes; l++) lanes_.push_back(Lane{OutRoute(gmax), z, z, z, z});
}

// the stage's one-time making, with its tables, state store and lane buffers, by the first call that needs it: under capture_mutex(), since
// an allocation must not land inside another thread's stream capture
template <class L> typename L::stage_type& OutChain::ensure(L& l, size_t lane_elems) {
    if (!l.stage) {
        std::lock_guard<std::mutex> cap(capture_mutex());
        l.lane.resize(lane_elems ? (size_t)n_lanes_ : 0);
        for (auto& b : l.lane) b.alloc(lane_elems);
        l.stage.reset(new typename L::stage_type(n_streams_, gmax_, &count_));
    }
    return *l.stage;
}

void OutChain::run(hipStream_t st, int lane, int G, int T, const int32_t* streams, float* native, const OutSpec* out, const LoudDst* loud,
                   float* const* dst, int64_t* n_out) {
    Lane& L = lanes_[(size_t)lane];
    OutRoute& r = L.route;
    if (const char* why = out_route(out, G, T, region(), loud_rows(), &r)) throw Error(why);
    if (r.any_metered) {   // reads the chunk as the output conv wrote it
        for (int g = 0; g < G; g++) {
            Q3_CHECK(!r.metered[g] || (loud && loud[g].rows), "a metered stream needs a place for its rows");
            L.lpos[g] = r.metered[g] ? loud[g].pos : 0;
        }
        LoudnessStage& m = ensure(loud_, (size_t)gmax_ * loud_rows() * 2);
        launch_loudness(st, m, native, G, T, streams, r.metered.data(), L.lpos.data(), loud_.lane[lane].p, r.loff.data(), L.lcnt.data());
        Q3_LAUNCH_CHECK();
        for (int g = 0; g < G; g++) {
            if (!r.metered[g] || L.lcnt[g] <= 0) continue;
            Q3_CHECK((size_t)L.lcnt[g] <= loud_rows(), "a pass completed more blocks than the meter's buffer holds");
            Q3_HIP(hipMemcpyAsync(loud[g].rows, reinterpret_cast<const unsigned char*>(loud_.lane[lane].p) + r.loff[g], (size_t)L.lcnt[g] * 2 * sizeof(double), hipMemcpyDeviceToHost, st));
        }
    }
    if (r.any_volume) {   // in place, in front of every stage below
        launch_volume(st, ensure(vol_, 0), native, G, T, streams, r.vol.data());   // no lane buffers: nothing else of vol_ is read here
        Q3_LAUNCH_CHECK();
    }
    for (int g = 0; g < G; g++) L.cnt[g] = L.scnt[g] = T;
    if (r.run[OUT_CONVERTED]) {
        PcmConverter& c = ensure(conv_, lane_floats_);
        launch_pcm_convert(st, c, native, G, T, streams, r.cf.data(), conv_.lane[lane].p, nullptr, L.cnt.data());
        Q3_LAUNCH_CHECK();
    }
    // the stretcher sets T for every stream it leaves alone and the shifter sets its own streams' counts only: they share scnt in this order
    if (r.run[OUT_RATED]) {
        TsmStretcher& s = ensure(tsm_, (size_t)gmax_ * region());
        launch_tsm_stretch(st, s, native, G, T, false, streams, r.pct.data(), r.enc.data(), tsm_.lane[lane].p, r.toff.data(), L.scnt.data());
        Q3_LAUNCH_CHECK();
    }
    if (r.run[OUT_PITCHED]) {
        PitchShifter& s = ensure(pitch_, (size_t)gmax_ * region());
        launch_tsm_pitch(st, s, native, G, T, false, streams, r.pr.data(), r.pp.data(), r.enc.data(), pitch_.lane[lane].p, r.toff.data(), L.scnt.data());
        Q3_LAUNCH_CHECK();
    }
    // every stream's bytes go out from where its stage left them (by OutKind; a stage that does not exist is nobody's source)
    const float* const base[4] = {native, conv_.stage ? conv_.lane[lane].p : nullptr, tsm_.stage ? tsm_.lane[lane].p : nullptr,
                                  pitch_.stage ? pitch_.lane[lane].p : nullptr};
    for (int g = 0; g < G; g++) {
        if (r.src[g] >= OUT_RATED) {
            prosody_[(size_t)streams[g]] = Prosody{out[g], true};
            L.cnt[g] = L.scnt[g];
            Q3_CHECK((size_t)L.cnt[g] <= region(), "a pass delivered more than the stage's buffer holds");
        }
        if (L.cnt[g] > 0) Q3_HIP(hipMemcpyAsync(dst[g], base[r.src[g]] + r.src_off[g], (size_t)L.cnt[g] * r.bytes[g], hipMemcpyDeviceToHost, st));
        if (n_out) n_out[g] = L.cnt[g];
    }
}

void OutChain::flush(hipStream_t st, int lane, int s, void* dst, int64_t* n_out) {
    *n_out = 0;
    if (!prosody_[(size_t)s].live) return;
    const OutSpec o = prosody_[(size_t)s].out;
    const bool pitched = out_kind(o) == OUT_PITCHED;
    const int32_t sl = s;
    const int64_t off = 0;
    // a live stream's stage exists: run made it
    if (pitched) launch_tsm_pitch(st, *pitch_.stage, nullptr, 1, 0, true, &sl, &o.rate_pct, &o.pitch_pct, &o.fmt.encoding, pitch_.lane[lane].p, &off, n_out);
    else launch_tsm_stretch(st, *tsm_.stage, nullptr, 1, 0, true, &sl, &o.rate_pct, &o.fmt.encoding, tsm_.lane[lane].p, &off, n_out);
    Q3_LAUNCH_CHECK();
    Q3_CHECK((size_t)*n_out <= region(), "flush larger than the stage's buffer");
    if (*n_out > 0) Q3_HIP(hipMemcpyAsync(dst, (pitched ? pitch_.lane : tsm_.lane)[lane].p, (size_t)*n_out * out_sample_bytes(o), hipMemcpyDeviceToHost, st));
    prosody_[(size_t)s].live = false; // flushed: the stream is reset before it is used again
}

void OutChain::reset_prosody(hipStream_t st, int s) {
    if (loud_.stage) loud_.stage->reset_async(st, s);
    if (tsm_.stage) tsm_.stage->reset_async(st, s);
    if (pitch_.stage) pitch_.stage->reset_async(st, s);
    if (vol_.stage) vol_.stage->reset_async(st, s);
    prosody_[(size_t)s] = Prosody{};
}

void OutChain::reset(hipStream_t st, int s) {
    if (conv_.stage) conv_.stage->reset_async(st, s); // the converter's history is part of the stream (one made later starts from zeros)
    reset_prosody(st, s);
}

void OutChain::restore(hipStream_t st, int s, const float* pcm_tail) {
    if (pcm_tail) { // the stream is delivered converted: its converter history is the preamble's last Q3_PCM_HIST native samples, not zeros
        PcmConverter& c = ensure(conv_, lane_floats_);
        c.check_slot(s);
        Q3_HIP(hipMemcpyAsync(c.hist + ((size_t)s * 2 + c.parity[(size_t)s]) * Q3_PCM_HIST, pcm_tail, sizeof(float) * Q3_PCM_HIST, hipMemcpyHostToDevice, st));
    }
    reset_prosody(st, s);
}

} // namespace q3
