// host_pack_check -- the library's host-only half (csrc/rtx_pack.hip) as a stand-alone program, so that its index arithmetic
// (t.local[idx], t.tri_rec[k], t.slot[...], the level tables) can run under AddressSanitizer and UBSan: built from this file and
// rtx_pack.hip alone, host-only, with -DRTX_LAB, and linked without the HIP runtime (tests/test_host_pack_sanitized.py).
//
//   host_pack_check CASE...
//
// A case file is flat and little-endian: four u64 {n_objects, n, mode, split}, then n_objects RtxObject (136 bytes each), then n u64
// indices, then the n RtxObject that replace them.  Each case runs host_refit -- what rtx_debug_host_refit_mesh runs: pack_scene,
// make_refit_tables, plan_update, the derivations, refit_packed or a re-pack, check_packed; split > 0: entries [0, split) are one
// update, the rest a second one -- and prints one line:
//   <file> status <RtxStatus> how <RTX_UPDATED_*> digests <16 hex words>       or       <file> status <RtxStatus> error <message>
// After a case that ran, the same scene goes through one hide / show round trip (host_visibility: what rtx_debug_host_set_visible runs)
// of its first seven objects and the update's indices; a line is printed only when the base pack's digests do not come back.
// A refusal plan_update documents (a bad index, an unknown kind or mode) is such a line and no failure.  The exit status is 1 when a
// case file is malformed or check_packed's walk found a broken invariant (its messages start with "bvh check:").
#include "../rust-raytracing_amd/csrc/rtx_pack.h"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>

int main(int argc, char **argv)
{
    int failed = 0;
    for (int a = 1; a < argc; ++a) {
        std::ifstream in(argv[a], std::ios::binary);
        const std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        uint64_t head[4] = { 0, 0, 0, 0 };                    // n_objects, n, mode, split
        if (raw.size() >= sizeof head) std::memcpy(head, raw.data(), sizeof head);
        const uint64_t room = raw.size() >= sizeof head ? raw.size() - sizeof head : 0;
        if (!in || raw.size() < sizeof head || head[0] > room / sizeof(RtxObject) || head[1] > room / (sizeof(RtxObject) + 8) ||
            head[0] * sizeof(RtxObject) + head[1] * (sizeof(RtxObject) + 8) != room || head[2] > 0xFFFFu || head[3] > 0xFFFFu) {
            std::printf("%s malformed\n", argv[a]);
            failed = 1;
            continue;
        }
        std::vector<RtxObject> objects(head[0]), updates(head[1]);
        std::vector<uint64_t> indices(head[1]);
        const char *at = raw.data() + sizeof head;
        if (head[0]) std::memcpy(objects.data(), at, head[0] * sizeof(RtxObject));
        at += head[0] * sizeof(RtxObject);
        if (head[1]) std::memcpy(indices.data(), at, head[1] * 8);
        if (head[1]) std::memcpy(updates.data(), at + head[1] * 8, head[1] * sizeof(RtxObject));
        RtxScene scene{};
        scene.n_objects = head[0];
        scene.objects = objects.data();
        uint64_t stats[16], digests[16];
        uint32_t how = 0;
        double info[8];
        const int32_t rc = rtx::host::host_refit("host_pack_check", &scene, indices.data(), updates.data(), head[1],
                                                 (uint32_t)(head[2] | (head[3] << 16)), stats, &how, digests, info);
        if (rc != RTX_OK) {
            const std::string &msg = rtx::host::last_error();
            std::printf("%s status %d error %s\n", argv[a], (int)rc, msg.c_str());
            if (msg.compare(0, 10, "bvh check:") == 0) failed = 1;
            continue;
        }
        std::printf("%s status 0 how %u digests", argv[a], how);
        for (uint64_t d : digests) std::printf(" %016llx", (unsigned long long)d);
        std::printf("\n");
        // one hide / show round trip of the scene's first objects and of the update's indices (rtx_scene_set_visible's host half:
        // plan_visibility, the kept words, hide_record, the refit with empty slots): the digests of the base pack must come back.
        // Nothing is printed unless they do not.
        std::vector<uint64_t> hide;
        for (uint64_t k = 0; k < head[0] && k < 7; ++k) hide.push_back(k);
        for (uint64_t k = 0; k < head[1]; ++k) if (indices[k] < head[0]) hide.push_back(indices[k]);
        std::vector<uint64_t> twice(hide);
        twice.insert(twice.end(), hide.rbegin(), hide.rend());
        const uint32_t kinds[2] = { rtx::host::kHostStepHide, rtx::host::kHostStepShow };
        const uint64_t begin[3] = { 0, hide.size(), twice.size() };
        uint32_t hows[2] = { 0, 0 };
        uint64_t base[16], back[16];
        std::vector<uint8_t> mask(head[0] + 1, 0);
        int32_t vrc = rtx::host::host_visibility("host_pack_check", &scene, kinds, begin, 0, nullptr, nullptr, hows, stats, base, nullptr, nullptr, nullptr, 0);
        if (vrc == RTX_OK)
            vrc = rtx::host::host_visibility("host_pack_check", &scene, kinds, begin, 2, twice.data(), nullptr, hows, stats, back, info, mask.data(), nullptr, 0);
        if (vrc != RTX_OK || std::memcmp(base, back, sizeof base) != 0) {
            std::printf("%s hide/show round trip: status %d how %u %u%s %s\n", argv[a], (int)vrc, hows[0], hows[1],
                        vrc == RTX_OK ? " digests differ" : "", vrc == RTX_OK ? "" : rtx::host::last_error().c_str());
            failed = 1;
        }
    }
    return failed;
}
