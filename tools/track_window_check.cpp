// Stand-alone host check of the window tracker (swk_tracker_*, swk_track_window in swiftwatcher_amd/csrc/tracker.cpp), meant to be
// compiled TOGETHER with tracker.cpp under the host sanitizers and run on a CPU machine -- it is not part of libswk.so, not loaded
// into Python and needs no GPU:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I include tools/track_window_check.cpp
//       swiftwatcher_amd/csrc/tracker.cpp -o track_window_check && ./track_window_check          (one command line)
//
// It feeds seeded streams of flying points through two handles: one takes them in windows of changing length with event buffers
// that start too small (every SWK_ERR_CAPACITY is answered by a second call with the sizes it reported), the other takes them one
// frame per call with ample buffers and is, every few windows, exported and imported into a fresh handle.  Both must report the
// same events (as paths of centroids: an import renumbers the segments).  It also walks the argument errors, the forced
// assignment that leaves a segment without a status, and a centroid outside the mask.  Prints a summary line; exit status 0 = clean.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <map>
#include <vector>
#include "swk_debug.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

namespace {

struct Rng {          // xorshift64*: the same stream on every machine
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
    uint64_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 0x2545F4914F6CDD1Dull; }
    double uniform() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
    int below(int n) { return (int)(uniform() * n); }
};

typedef std::pair<double, double> Point;
typedef std::vector<Point> Path;

struct Stream {
    std::vector<int32_t> nseg;
    std::vector<double> cents;          // (row, col) pairs, frame after frame
    std::vector<size_t> start;          // first segment of each frame
};

Stream make_stream(Rng &rng, int H, int W, int nframes, bool snap)
{
    struct Bird { double r, c, vr, vc; };
    std::vector<Bird> birds;
    Stream s;
    size_t total = 0;
    for (int f = 0; f < nframes; ++f) {
        std::vector<Bird> kept;
        for (Bird b : birds) {
            if (rng.uniform() < 0.12) continue;
            b.r += b.vr + rng.uniform() - 0.5;
            b.c += b.vc + rng.uniform() - 0.5;
            if (b.r >= 0 && b.r < H && b.c >= 0 && b.c < W) kept.push_back(b);
        }
        birds.swap(kept);
        while (birds.size() < 12 && rng.uniform() < 0.45)
            birds.push_back({rng.uniform() * H, rng.uniform() * W, rng.uniform() * 10 - 5, rng.uniform() * 10 - 5});
        if (rng.uniform() < 0.08) birds.clear();
        s.start.push_back(total);
        s.nseg.push_back((int32_t)birds.size());
        for (const Bird &b : birds) {
            s.cents.push_back(snap ? (double)((int)b.r / 4 * 4) : b.r);
            s.cents.push_back(snap ? (double)((int)b.c / 4 * 4) : b.c);
        }
        total += birds.size();
    }
    s.start.push_back(total);
    return s;
}

// A handle plus the caller's side of the ordinals: the centroid of every segment a later event can still name.
struct Side {
    swk_tracker *t = nullptr;
    std::map<int64_t, Point> known;
    std::vector<Path> events;
    int64_t retries = 0;

    void run(const Stream &s, int from, int count, int32_t ev_cap, int64_t ord_cap)
    {
        std::vector<int64_t> off((size_t)ev_cap + 1), ords((size_t)ord_cap);
        int32_t n_events = 0, done = 0;
        int64_t n_ords = 0, first = 0, min_live = 0;
        const double *c = s.cents.data() + 2 * s.start[from];
        int32_t rc = swk_track_window(t, count, s.nseg.data() + from, c, ev_cap, ord_cap, off.data(), ords.data(), &n_events, &n_ords,
                                      &done, &first, &min_live);
        if (rc == SWK_ERR_CAPACITY) {
            ++retries;
            CHECK(n_events > ev_cap || n_ords > ord_cap);
            off.assign((size_t)n_events + 1, 0);
            ords.assign((size_t)n_ords, 0);
            rc = swk_track_window(t, count, s.nseg.data() + from, c, n_events, n_ords, off.data(), ords.data(), &n_events, &n_ords, &done,
                                  &first, &min_live);
        }
        CHECK(rc == SWK_OK && done == count);
        const size_t segs = s.start[from + count] - s.start[from];
        for (size_t k = 0; k < segs; ++k) known[first + (int64_t)k] = Point(c[2 * k], c[2 * k + 1]);
        CHECK(off[0] == 0 && off[n_events] == n_ords);
        for (int32_t e = 0; e < n_events; ++e) {
            Path p;
            for (int64_t k = off[e]; k < off[e + 1]; ++k) {
                CHECK(known.count(ords[k]) == 1);
                p.push_back(known[ords[k]]);
            }
            CHECK(p.size() >= 2);
            events.push_back(p);
        }
        CHECK(min_live <= first + (int64_t)segs);
        known.erase(known.begin(), known.lower_bound(min_live));          // what the call says can be let go
    }

    // export the live state, import it into a fresh handle and go on with that one
    void transplant(const uint8_t *roi, int H, int W)
    {
        int32_t n = 0;
        int64_t n_ords = 0;
        int64_t dummy_off = 0;
        int32_t rc = swk_tracker_export(t, 0, 0, nullptr, nullptr, &dummy_off, nullptr, &n, &n_ords);
        CHECK(rc == (n || n_ords ? SWK_ERR_CAPACITY : SWK_OK));
        std::vector<double> cents(2 * (size_t)n), first(2 * (size_t)n);
        std::vector<int64_t> ords((size_t)n), off((size_t)n + 1), chain((size_t)n_ords), lens((size_t)n);
        CHECK(swk_tracker_export(t, n, n_ords, cents.data(), ords.data(), off.data(), chain.data(), &n, &n_ords) == SWK_OK);
        for (int32_t k = 0; k < n; ++k) {
            lens[k] = off[k + 1] - off[k];
            if (lens[k]) { first[2 * k] = known[chain[off[k]]].first; first[2 * k + 1] = known[chain[off[k]]].second; }
        }
        swk_tracker *fresh = nullptr;
        CHECK(swk_tracker_create(roi, H, W, &fresh) == SWK_OK);
        int64_t base = -1;
        CHECK(swk_tracker_import(fresh, n, cents.data(), lens.data(), first.data(), &base) == SWK_OK && base == 0);
        std::map<int64_t, Point> renumbered;
        int64_t at = base;
        for (int32_t k = 0; k < n; ++k)
            for (int64_t m = off[k]; m < off[k + 1]; ++m) { CHECK(known.count(chain[m]) == 1); renumbered[at++] = known[chain[m]]; }
        for (int32_t k = 0; k < n; ++k) renumbered[at++] = Point(cents[2 * k], cents[2 * k + 1]);
        known.swap(renumbered);
        swk_tracker_destroy(t);
        t = fresh;
    }
};

void argument_errors(const uint8_t *roi, int H, int W)
{
    swk_tracker *t = nullptr;
    CHECK(swk_tracker_create(nullptr, H, W, &t) == SWK_ERR_ARG && t == nullptr);
    CHECK(swk_tracker_create(roi, -1, W, &t) == SWK_ERR_ARG);
    CHECK(swk_tracker_create(roi, H, W, nullptr) == SWK_ERR_ARG);
    CHECK(swk_tracker_create(roi, H, W, &t) == SWK_OK);
    int32_t nseg[2] = {1, -1}, n_events = 0, done = 0;
    double cents[4] = {1, 1, 2, 2};
    int64_t off[4], ords[4], n_ords = 0, first = 0, min_live = 0;
    CHECK(swk_track_window(nullptr, 0, nullptr, nullptr, 3, 4, off, ords, &n_events, &n_ords, &done, &first, &min_live) == SWK_ERR_ARG);
    CHECK(swk_track_window(t, -1, nseg, cents, 3, 4, off, ords, &n_events, &n_ords, &done, &first, &min_live) == SWK_ERR_ARG);
    CHECK(swk_track_window(t, 2, nseg, cents, 3, 4, off, ords, &n_events, &n_ords, &done, &first, &min_live) == SWK_ERR_ARG);
    CHECK(swk_track_window(t, 1, nullptr, cents, 3, 4, off, ords, &n_events, &n_ords, &done, &first, &min_live) == SWK_ERR_ARG);
    CHECK(swk_track_window(t, 1, nseg, nullptr, 3, 4, off, ords, &n_events, &n_ords, &done, &first, &min_live) == SWK_ERR_ARG);
    CHECK(swk_track_window(t, 1, nseg, cents, 3, 4, nullptr, ords, &n_events, &n_ords, &done, &first, &min_live) == SWK_ERR_ARG);
    CHECK(swk_track_window(t, 0, nullptr, nullptr, 0, 0, off, nullptr, &n_events, &n_ords, &done, nullptr, nullptr) == SWK_OK);
    int64_t lens[1] = {-1};
    CHECK(swk_tracker_import(t, 1, cents, lens, cents, nullptr) == SWK_ERR_ARG);
    CHECK(swk_tracker_import(t, -1, nullptr, nullptr, nullptr, nullptr) == SWK_ERR_ARG);
    CHECK(swk_tracker_import(t, 0, nullptr, nullptr, nullptr, nullptr) == SWK_OK);
    // a forced assignment that puts both current segments off their diagonal: the frame before it is applied, that one is not
    int32_t two[3] = {1, 2, 1}, swapped[2] = {1, 0}, bad[2] = {0, 2};
    double pts[10] = {5, 5, 6, 6, 20, 20, 7, 7, 21, 21};
    CHECK(swk_debug_tracker_force_assignment(t, 0, bad, 2) == SWK_ERR_ARG);
    CHECK(swk_debug_tracker_force_assignment(t, 1, swapped, 2) == SWK_OK);
    CHECK(swk_track_window(t, 1, two, pts, 3, 4, off, ords, &n_events, &n_ords, &done, &first, &min_live) == SWK_OK && done == 1);
    swk_tracker *u = nullptr;                                   // (an empty state, so that the frame has no previous segments)
    CHECK(swk_tracker_create(roi, H, W, &u) == SWK_OK);
    CHECK(swk_debug_tracker_force_assignment(u, 1, swapped, 2) == SWK_OK);
    int32_t frames[3] = {0, 2, 1};
    CHECK(swk_track_window(u, 3, frames, pts + 2, 3, 4, off, ords, &n_events, &n_ords, &done, &first, &min_live) == SWK_ERR_TRACK_STATUS);
    CHECK(done == 1 && n_events == 0);
    CHECK(swk_track_window(u, 2, frames + 1, pts + 2, 3, 4, off, ords, &n_events, &n_ords, &done, &first, &min_live) == SWK_OK && done == 2);
    // a vanished segment outside the mask: refused, nothing applied
    double outside[2] = {(double)H + 3, 1};
    int32_t one_then_none[2] = {1, 0};
    CHECK(swk_track_window(u, 2, one_then_none, outside, 3, 4, off, ords, &n_events, &n_ords, &done, &first, &min_live) == SWK_ERR_ARG);
    int32_t n = 0;
    CHECK(swk_tracker_export(u, 0, 0, nullptr, nullptr, off, nullptr, &n, &n_ords) == SWK_ERR_CAPACITY && n == 1);
    swk_tracker_destroy(u);
    swk_tracker_destroy(t);
    swk_tracker_destroy(nullptr);
}

}  // namespace

int main()
{
    const int H = 64, W = 96;
    long total_events = 0, total_retries = 0, transplants = 0;
    for (int stream = 0; stream < 60; ++stream) {
        Rng rng(1234 + stream);
        std::vector<uint8_t> roi((size_t)H * W, 0);
        const int r0 = rng.below(H - 8), c0 = rng.below(W - 8), r1 = r0 + 8 + rng.below(H), c1 = c0 + 8 + rng.below(W);
        for (int r = r0; r < r1 && r < H; ++r)
            for (int c = c0; c < c1 && c < W; ++c) roi[(size_t)r * W + c] = 255;
        if (stream == 0) argument_errors(roi.data(), H, W);
        const Stream s = make_stream(rng, H, W, 240, stream % 2 == 1);
        Side windows, frames;
        CHECK(swk_tracker_create(roi.data(), H, W, &windows.t) == SWK_OK);
        CHECK(swk_tracker_create(roi.data(), H, W, &frames.t) == SWK_OK);
        int at = 0, chunk = 0;
        while (at < 240) {
            const int count = std::min(240 - at, rng.below(30));          // 0 frames is a valid window
            windows.run(s, at, count, 0, 0);                              // buffers that start too small whenever there is an event
            for (int f = at; f < at + count; ++f) frames.run(s, f, 1, 64, 4096);
            if (++chunk % 3 == 0) { frames.transplant(roi.data(), H, W); ++transplants; }
            at += count;
        }
        windows.run(s, 0, 0, 0, 0);
        int32_t none[4] = {0, 0, 0, 0};                                   // the null frames at a video's end
        Stream tail;
        tail.nseg.assign(none, none + 4);
        tail.start.assign(5, 0);
        tail.cents.assign(2, 0.0);
        windows.run(tail, 0, 4, 0, 0);
        frames.run(tail, 0, 4, 64, 4096);
        CHECK(windows.events == frames.events);
        CHECK(frames.retries == 0);
        total_events += (long)windows.events.size();
        total_retries += (long)windows.retries;
        swk_tracker_destroy(windows.t);
        swk_tracker_destroy(frames.t);
    }
    CHECK(total_events > 500 && total_retries > 200 && transplants > 100);
    printf("track_window_check: 60 streams, %ld events, %ld capacity retries, %ld export/import transplants: clean\n", total_events,
           total_retries, transplants);
    return 0;
}
