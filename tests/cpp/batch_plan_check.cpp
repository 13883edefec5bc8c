// batch_plan_check - prints what the launch policy (extractorb_amd/csrc/orbx_batch_plan.hpp) makes of a geometry and a call, without a device.
// Built by tests/test_batch_plan.py with g++ and only -I csrc -I include: that it builds shows the header is host only.
//
// stdin: one case per line, key=value tokens (any order; a missing key keeps its default):
//   rows cols nf nlevels sf maxB                                              the extractor and its image
//   numCUs pyrCols fastWide patchBlur blurSplit colsShape splitMode fuseSmall splitMinPixels leafFrames octForced octRoomy bytewise arena
//                                                                             LaunchPolicy as orbx_create would fill it
//   lastBlurForm lastSplitLevel blurOwed      the state the earlier call left; prev=1 takes what the previous LINE's call left instead
//   profiling B stages                        the call
// stdout: one JSON object per line: the geometry's facts, the GeometryPlan, the BatchPlan, the FrontPlan (if the call has a front), the BackPlan
// of every part (two where the tails are staggered), the state the call leaves and what orbx_debug_last_forms / orbx_profile_kernel_name_of
// would report after it.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "orbx_batch_plan.hpp"

using namespace orbx;

static void ints(const char* key, const int* v, int n) {
    std::printf("\"%s\": [", key);
    for (int i = 0; i < n; i++) std::printf("%s%d", i ? ", " : "", v[i]);
    std::printf("]");
}

int main() {
    std::string line;
    CallState left;      // what the previous line's call left
    std::string resizeName, fastName, octName;      // the kernel names as the handle would hold them
    int pyrForm = -1, pyrCut = 0;
    FrameGeom g;
    std::string geomKey, why, checkedTables;
    while (std::getline(std::cin, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::map<std::string, double> kv;
        std::istringstream in(line);
        for (std::string tok; in >> tok;) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) { std::fprintf(stderr, "bad token %s\n", tok.c_str()); return 2; }
            kv[tok.substr(0, eq)] = std::atof(tok.c_str() + eq + 1);
        }
        auto get = [&](const char* k, double dflt) { auto it = kv.find(k); return it == kv.end() ? dflt : it->second; };
        const int rows = (int)get("rows", 480), cols = (int)get("cols", 640), nlevels = (int)get("nlevels", 8), maxB = (int)get("maxB", 1);
        LaunchPolicy p;
        p.nfeatures = (int)get("nf", 1000);
        p.numCUs = (int)get("numCUs", 256);
        p.pyrCols = (int)get("pyrCols", -1); p.fastWide = (int)get("fastWide", -1); p.patchBlur = (int)get("patchBlur", -1);
        p.blurSplit = (int)get("blurSplit", -1); p.colsShape = (int)get("colsShape", -1); p.splitMode = (int)get("splitMode", 1);
        p.fuseSmall = get("fuseSmall", 1) != 0; p.splitMinPixels = (long long)get("splitMinPixels", 120e6);
        p.leafFrames = (int)get("leafFrames", 0); p.octThreadsForced = (int)get("octForced", 0); p.octRoomyForced = get("octRoomy", 0) != 0;
        p.resizeBytewise = get("bytewise", 0) != 0; p.octArena = get("arena", 0) != 0;
        CallState s;
        if (get("prev", 0) != 0) s = left;
        else {
            s.lastBlurForm = (int)get("lastBlurForm", -1); s.lastSplitLevel = (int)get("lastSplitLevel", 0); s.blurOwed = get("blurOwed", 0) != 0;
            resizeName = fastName = octName = ""; pyrForm = -1; pyrCut = 0;
        }
        s.profiling = get("profiling", 0) != 0;
        const int B = (int)get("B", 1), stages = (int)get("stages", kStageFront | kStageBack);

        char key[128];
        std::snprintf(key, sizeof key, "%d %d %d %d %.9g %d", rows, cols, p.nfeatures, nlevels, get("sf", 1.2), maxB);
        if (geomKey != key) {      // (lines of one extractor follow each other: its geometry is built once)
            why = makeFrameGeom(makeScaleTables(p.nfeatures, (float)get("sf", 1.2), nlevels), rows, cols, g);
            if (why.empty()) layoutArenas(g, maxB);
            geomKey = key;
        }
        if (!why.empty()) { std::printf("{\"refused\": \"%s\"}\n", why.c_str()); continue; }
        const GeometryPlan gp = planGeometry(g, p);
        const std::string tablesKey = geomKey + " " + std::to_string(gp.splitLevel);
        if (tablesKey != checkedTables) {   // the tables the library stages are the ones the plan counted (they depend on the geometry and the split level)
            checkedTables = tablesKey;
            std::vector<BlurItem> items;
            std::vector<unsigned short> laneItem;
            if (!buildBlurTables(g, gp, items, laneItem)) { checkedTables.clear(); std::printf("{\"refused\": \"blur item table does not fit\"}\n"); continue; }
            size_t ni = 0, nl = 0;
            for (int v = 0; v < 3; v++) {
                if (gp.blurItemOff[v] != ni || gp.blurLaneOff[v] != nl || (gp.nBlurItems[v] && items[ni].count != gp.nBlurItems[v])) { std::fprintf(stderr, "blur table %d: offsets\n", v); return 1; }
                for (int i = 0; i < gp.nBlurItems[v]; i++) {
                    const BlurItem& it = items[ni + i];
                    const int n = (g.lv[it.level].w + 3) / 4;
                    if (it.firstLane < 0 || it.firstLane + n > gp.nBlurLanes[v]) { std::fprintf(stderr, "blur table %d: lanes\n", v); return 1; }
                    for (int k = 0; k < n; k++) if (laneItem[nl + it.firstLane + k] != i) { std::fprintf(stderr, "blur table %d: lane item\n", v); return 1; }
                }
                ni += gp.nBlurItems[v]; nl += gp.nBlurLanes[v];
            }
            if (ni != items.size() || nl != laneItem.size()) { std::fprintf(stderr, "blur tables: sizes\n"); return 1; }
        }
        int w[kMaxLevels], hh[kMaxLevels], quota[kMaxLevels];
        for (int l = 0; l < g.nlevels; l++) { w[l] = g.lv[l].w; hh[l] = g.lv[l].h; quota[l] = g.lv[l].quota; }
        std::printf("{\"geom\": {\"nlevels\": %d, ", g.nlevels);
        ints("w", w, g.nlevels); std::printf(", "); ints("h", hh, g.nlevels); std::printf(", "); ints("quota", quota, g.nlevels);
        std::printf(", \"sumPixels\": %lld, \"cells\": %d, \"maxRoiW\": %d, \"maxRoiH\": %d, \"big\": %d, \"colsPacked\": %d, \"cuts\": [", g.sumPixels,
                    (int)g.cells.size(), g.maxRoiW, g.maxRoiH, (int)g.big, (int)g.colsPacked);
        for (size_t i = 0; i < g.colSets.size(); i++)
            std::printf("%s{\"px\": %d, \"regions\": %d, \"fit\": %d, \"ldsBytes\": %d}", i ? ", " : "", g.colSets[i].px, (int)g.colSets[i].columns.size(), (int)g.colSets[i].fit, g.colSets[i].ldsBytes);
        std::printf("]}, \"geometryPlan\": {\"splitLevel\": %d, \"octThreads\": %d, ", gp.splitLevel, gp.octThreads);
        ints("nBlurLanes", gp.nBlurLanes, 3); std::printf(", "); ints("nBlurItems", gp.nBlurItems, 3);
        std::printf(", \"blurItemOff\": [%zu, %zu, %zu], \"blurLaneOff\": [%zu, %zu, %zu]}", gp.blurItemOff[0], gp.blurItemOff[1], gp.blurItemOff[2],
                    gp.blurLaneOff[0], gp.blurLaneOff[1], gp.blurLaneOff[2]);

        const BatchPlan b = planBatch(g, gp, p, s, B, stages);
        std::printf(", \"batch\": {\"bigBatch\": %d, \"patchBlur\": %d, \"splitL\": %d, \"blurSide\": %d, \"stagger\": %d, \"B0\": %d}", (int)b.bigBatch,
                    (int)b.patchBlur, b.splitL, (int)b.blurSide, (int)b.stagger, b.B0);
        left = s;
        if (stages & kStageFront) {
            const FrontPlan f = planFront(g, gp, p, s, b, B);
            std::printf(", \"front\": {\"cut\": %d, \"cutPx\": %d, \"pyrForm\": %d, \"colsShape\": %d, \"resizeKernel\": \"%s\", \"blurForm\": %d, \"blurTable\": %d, "
                        "\"blurBlockRows\": %d, \"blurOwed\": %d}", f.cut, f.cut >= 0 ? g.colSets[f.cut].px : 0, f.pyrForm(), f.colsShape, f.resizeKernel,
                        f.blurForm, f.blurTable, f.blurBlockRows, (int)f.blurOwed);
            left.lastBlurForm = f.blurForm; left.lastSplitLevel = b.splitL; left.blurOwed = f.blurOwed;
            pyrForm = f.pyrForm(); pyrCut = f.cut >= 0 ? g.colSets[f.cut].px : 0;
            if (f.cut >= 0 || g.nlevels > 2) resizeName = f.resizeKernel;
        }
        if (stages & kStageBack) {
            std::printf(", \"back\": [");
            const int nParts = b.stagger ? 2 : 1;
            for (int i = 0; i < nParts; i++) {
                const int f0 = i ? b.B0 : 0, Bn = b.stagger ? (i ? B - b.B0 : b.B0) : B;
                const BackPlan k = planBack(g, gp, p, s, f0, Bn, left.blurOwed);
                left.blurOwed = false;
                std::printf("%s{\"f0\": %d, \"Bn\": %d, \"leafTables\": %d, \"carry\": %d, \"blurFirst\": %d, \"wide\": %d, \"fastKernel\": \"%s\", ", i ? ", " : "", f0, Bn,
                            (int)k.leafTables, (int)k.carry, (int)k.blurFirst, (int)k.wide, k.fastKernel);
                ints("octT", k.octT, g.nlevels);
                std::printf(", \"roomy\": %d, \"octKernel\": \"%s\"}", (int)k.roomy, k.octKernel);
                fastName = k.fastKernel; octName = k.octKernel;
            }
            std::printf("]");
        }
        std::printf(", \"left\": {\"lastBlurForm\": %d, \"lastSplitLevel\": %d, \"blurOwed\": %d}", left.lastBlurForm, left.lastSplitLevel, (int)left.blurOwed);
        std::printf(", \"reported\": {\"pyr_form\": %d, \"cut_px\": %d, \"blur_form\": %d, \"split_level\": %d, \"resize\": \"%s\", \"fast\": \"%s\", \"octree\": \"%s\"}}\n",
                    pyrForm, pyrCut, left.lastBlurForm, left.lastBlurForm == kBlurSplitByLevel ? left.lastSplitLevel : 0, resizeName.c_str(), fastName.c_str(), octName.c_str());
    }
    return 0;
}
